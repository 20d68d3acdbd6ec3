"""Image metrics and `args.txt` parsing for the entry points (reference: core/utils/evaluation_helpers.py:221-385 and
run_render.py:1178-1263).

PSNR is the reference's formula.  SSIM: the reference imports a pinned fork of a third-party package
(`pytorch-msssim @ git+https://github.com/LemonATsu/pytorch-msssim.git@f77a2446`, requirements.txt:7) that returns the
per-pixel SSIM *map* -- the package is not in this image, so `ssim_map` restates the published algorithm (Wang et al. 2004 as
implemented by pytorch-msssim: 11-tap Gaussian window, sigma 1.5, K1 = 0.01, K2 = 0.03, separable filtering) with zero padding
so the map has the image's size.  **SSIM parity is unpinned** (no reference output to compare with); PSNR needs no third-party code.
What the reference's call sites fix about the fork (4-D image-sized map, default window, unit data range) and what they leave open
(the padding mode: only the 5-pixel border of the map depends on it) is written out in oracle/gen_ssim_golden.py, whose
known-answer vector pins this function's arithmetic (tests/test_host_logic.py).
"""
import numpy as np
import torch
import torch.nn.functional as F

from ..config import txt_to_argstring  # noqa: F401  (reference location of this helper)


def to8b(x):
    return (255 * np.clip(x, 0, 1)).astype(np.uint8)


def _gauss(size=11, sigma=1.5):
    x = torch.arange(size, dtype=torch.float32) - size // 2
    g = torch.exp(-(x ** 2) / (2 * sigma ** 2))
    return g / g.sum()


def _blur(x, g):
    C, p = x.shape[1], g.numel() // 2
    x = F.conv2d(x, g.view(1, 1, -1, 1).expand(C, 1, -1, 1), padding=(p, 0), groups=C)
    return F.conv2d(x, g.view(1, 1, 1, -1).expand(C, 1, 1, -1), padding=(0, p), groups=C)


def ssim_map(x, y, data_range=1.0, win_size=11, win_sigma=1.5, K=(0.01, 0.03)):
    """x, y [N,C,H,W] -> per-pixel, per-channel SSIM [N,C,H,W]"""
    g = _gauss(win_size, win_sigma).to(x.device, x.dtype)
    C1, C2 = (K[0] * data_range) ** 2, (K[1] * data_range) ** 2
    mu1, mu2 = _blur(x, g), _blur(y, g)
    s1, s2, s12 = _blur(x * x, g) - mu1 * mu1, _blur(y * y, g) - mu2 * mu2, _blur(x * y, g) - mu1 * mu2
    cs = (2 * s12 + C2) / (s1 + s2 + C2)
    return (2 * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1) * cs


def _masked_scores(sqr_diff, ssim, mask):
    """per-image PSNR / SSIM over the pixels of a [N,H,W,1] mask (x3 channels), inf -> 0, mean over images"""
    n = len(sqr_diff)
    denom = np.maximum(mask.reshape(n, -1).sum(-1) * 3., 1.)
    with np.errstate(divide='ignore'):
        psnr = -10. * np.log10((sqr_diff * mask).reshape(n, -1).sum(-1) / denom)
    ssim = (ssim * mask).reshape(n, -1).sum(-1) / denom
    psnr[psnr == np.inf] = 0.
    return float(psnr.mean()), float(ssim.mean())


def evaluate_metric(rgbs, gt_imgs, disps=None, gt_masks=None, valid_idxs=None, poses=None, kps=None, hwf=None, centers=None,
                    ext_scale=None, vid_base=None, eval_postfix="", eval_both=False, white_bkgd=False, render_factor=0, **_):
    """Validation scores of `render_testset` (reference evaluation_helpers.py:257-385): whole image when there is neither a
    foreground mask nor a valid-ray mask; foreground only when `gt_masks` is given; with `eval_both` the headline numbers are
    taken inside the cylinder boxes (`valid_idxs`) and the foreground ones are reported next to them.  Score files are appended
    under `vid_base` like the reference (videos are not written: no imageio in this image)."""
    rgbs, gt_imgs = np.asarray(rgbs, dtype=np.float32), np.asarray(gt_imgs, dtype=np.float32)
    H, W = gt_imgs.shape[1:3]
    valid_masks = None
    if eval_both:
        if valid_idxs is None or render_factor != 0:
            from .ray_utils import kp_to_valid_rays
            _, valid_idxs, _, _ = kp_to_valid_rays(poses, *hwf, centers=centers, kps=kps, ext_scale=ext_scale)
        valid_masks = np.zeros((len(valid_idxs), H * W, 1), dtype=np.float32)
        for i, idx in enumerate(valid_idxs):
            valid_masks[i, np.asarray(idx)] = 1
        valid_masks = valid_masks.reshape(-1, H, W, 1)
    if gt_masks is not None:
        keep = np.where(gt_masks.reshape(len(gt_masks), -1).sum(-1) > 0)[0]      # images with a person in them
        rgbs, gt_imgs, gt_masks = rgbs[keep], gt_imgs[keep], gt_masks[keep]
        valid_masks = valid_masks[keep] if valid_masks is not None else None
    th_rgbs = torch.tensor(rgbs).permute(0, 3, 1, 2)
    if render_factor > 0:
        th_rgbs = F.interpolate(th_rgbs, size=gt_imgs.shape[1:3], mode='bilinear', align_corners=False)
        rgbs = th_rgbs.permute(0, 2, 3, 1).numpy()
    ssim = ssim_map(th_rgbs, torch.tensor(gt_imgs).permute(0, 3, 1, 2)).permute(0, 2, 3, 1).numpy()
    sqr_diff = np.square(gt_imgs - rgbs)
    fg_psnr = fg_ssim = None
    if gt_masks is not None:
        fg_psnr, fg_ssim = _masked_scores(sqr_diff, ssim, gt_masks[..., :1])
    if valid_masks is None and gt_masks is None:
        psnr, ssim_v = _masked_scores(sqr_diff, ssim, np.ones_like(sqr_diff[..., :1]))
    elif valid_masks is not None:
        psnr, ssim_v = _masked_scores(sqr_diff, ssim, valid_masks)
    else:
        psnr, ssim_v = fg_psnr, fg_ssim
    if vid_base is not None:
        scores = [("psnr", psnr), ("ssim", ssim_v)]
        if valid_masks is not None and gt_masks is not None:
            scores += [("psnr_fg", fg_psnr), ("ssim_fg", fg_ssim)]
        for name, v in scores:
            base, _, fg = name.partition("_")
            with open(vid_base + f"{base}{eval_postfix}{'_fg' if fg else ''}.txt", "a") as f:
                f.write(f"{v}\n")
    return {"psnr": psnr, "ssim": ssim_v, "psnr_fg": fg_psnr, "ssim_fg": fg_ssim}


def evaluate_in_boxes(rgbs, accs, bboxes, gt_imgs, gt_masks=None, bg_imgs=None, bg_indices=None):
    """Per-frame scores inside each frame's 2-D cylinder box (reference run_render.py:1178-1263): box PSNR / SSIM and, with
    masks, foreground PSNR / SSIM; frames whose cropped mask is empty are skipped.  -> dict of lists"""
    out = {'psnr': [], 'ssim': [], 'fg_psnr': [], 'fg_ssim': []}
    for i, (rgb, (tl, br), gt) in enumerate(zip(rgbs, bboxes, gt_imgs)):
        gt = np.asarray(gt, dtype=np.float32).reshape(rgb.shape)
        mask = None
        if gt_masks is not None:
            mask = np.asarray(gt_masks[i], dtype=np.float32).reshape(*rgb.shape[:2], -1)[..., :1]
            if bg_imgs is not None:
                gt = gt * mask + (1. - mask) * bg_imgs[bg_indices[i]]
            mask = mask[tl[1]:br[1], tl[0]:br[0]]
            if mask.sum() < 1:
                continue
        g, r = gt[tl[1]:br[1], tl[0]:br[0]], np.asarray(rgb, dtype=np.float32)[tl[1]:br[1], tl[0]:br[0]]
        se = np.square(g - r)
        s = ssim_map(torch.tensor(r[None]).permute(0, 3, 1, 2), torch.tensor(g[None]).permute(0, 3, 1, 2))
        s = s.permute(0, 2, 3, 1).numpy()[0]
        out['psnr'].append(float(-10. * np.log10(se.mean())))
        out['ssim'].append(float(s.mean()))
        if mask is not None:
            denom = mask.sum() * 3.
            out['fg_psnr'].append(float(-10. * np.log10((se * mask).sum() / denom)))
            out['fg_ssim'].append(float((s * mask).sum() / denom))
    return out


# ------------------------------------------------------------------------------------------------ scoring on the device
# (--eval_device: hip_ops.image_metrics sums squared error and SSIM per image on the GPU; only those sums cross to the host.  The
# functions above stay the statement of what is computed.)
def scores_from_sums(sum_se, sum_ssim, denom, guard=True, inf_to_zero=True, mean=True):
    """PSNR / SSIM per image from the sums of squared error and SSIM over `denom` values each (pixels x 3, or mask weight x 3), in
    float64.  guard: `max(denom, 1)` as _masked_scores; inf_to_zero: a PSNR of inf (zero error) counts 0, the reference's convention
    in evaluate_metric (evaluate_in_boxes uses neither).  -> (psnr, ssim): floats, the mean over images, or with mean=False the
    per-image float64 arrays."""
    se, ss, d = (np.atleast_1d(np.asarray(x, dtype=np.float64)) for x in (sum_se, sum_ssim, denom))
    if guard:
        d = np.maximum(d, 1.)
    with np.errstate(divide='ignore', invalid='ignore'):
        psnr, ssim = -10. * np.log10(se / d), ss / d
    if inf_to_zero:
        psnr[psnr == np.inf] = 0.
    return (float(psnr.mean()), float(ssim.mean())) if mean else (psnr, ssim)


def _on_device(x, device, dtype=torch.float32):
    """a device tensor as it is, anything else uploaded once"""
    if torch.is_tensor(x):
        return x.to(device=device, dtype=dtype)
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).to(device)


def _device_of(x):
    if torch.is_tensor(x) and x.is_cuda:
        return x.device
    if not torch.cuda.is_available():
        raise RuntimeError("scoring on the device: no GPU visible -- libdanbo_hip has no CPU fallback")
    return torch.device('cuda', torch.cuda.current_device())


def evaluate_metric_device(rgbs, gt_imgs, disps=None, gt_masks=None, valid_idxs=None, poses=None, kps=None, hwf=None, centers=None,
                           ext_scale=None, vid_base=None, eval_postfix="", eval_both=False, white_bkgd=False, render_factor=0, **_):
    """evaluate_metric with the frames scored on the device: the same keywords, result dictionary and score files.  rgbs, gt_imgs,
    gt_masks are device tensors (as render_path(device_out=True) returns them) or arrays, uploaded once.  The valid-ray mask, the
    "images with a person" filter and the render_factor resize are torch on the device; the scoring is ONE hip_ops.image_metrics
    call with the valid mask as mask_a and the foreground as mask_b, and [N,8] sums are all that crosses to the host."""
    from .. import hip_ops
    dev = _device_of(rgbs)
    rgbs, gt_imgs = _on_device(rgbs, dev), _on_device(gt_imgs, dev)
    H, W = gt_imgs.shape[1:3]
    valid_masks = None
    if eval_both:
        if valid_idxs is None or render_factor != 0:
            from .ray_utils import kp_to_valid_rays
            _, valid_idxs, _, _ = kp_to_valid_rays(poses, *hwf, centers=centers, kps=kps, ext_scale=ext_scale)
        valid_masks = torch.zeros(len(valid_idxs), H * W, device=dev)
        for i, idx in enumerate(valid_idxs):
            valid_masks[i, torch.as_tensor(idx).to(dev).long()] = 1
        valid_masks = valid_masks.view(-1, H, W)
    if gt_masks is not None:
        gt_masks = _on_device(gt_masks, dev)
        gt_masks = gt_masks.reshape(len(gt_masks), H, W, -1)[..., 0]
        keep = torch.nonzero(gt_masks.reshape(len(gt_masks), -1).sum(-1) > 0)[:, 0]      # images with a person in them
        rgbs, gt_imgs, gt_masks = rgbs[keep], gt_imgs[keep], gt_masks[keep]
        valid_masks = valid_masks[keep] if valid_masks is not None else None
    if render_factor > 0:
        rgbs = F.interpolate(rgbs.permute(0, 3, 1, 2), size=(H, W), mode='bilinear', align_corners=False).permute(0, 2, 3, 1)
    s = hip_ops.image_metrics(rgbs, gt_imgs, mask_a=valid_masks, mask_b=gt_masks)['sums'].double().cpu().numpy()
    fg_psnr = fg_ssim = None
    if gt_masks is not None:
        fg_psnr, fg_ssim = scores_from_sums(s[:, 5], s[:, 6], s[:, 7] * 3.)
    if valid_masks is None and gt_masks is None:
        psnr, ssim_v = scores_from_sums(s[:, 0], s[:, 1], np.full(len(s), H * W * 3.))
    elif valid_masks is not None:
        psnr, ssim_v = scores_from_sums(s[:, 2], s[:, 3], s[:, 4] * 3.)
    else:
        psnr, ssim_v = fg_psnr, fg_ssim
    if vid_base is not None:
        scores = [("psnr", psnr), ("ssim", ssim_v)]
        if valid_masks is not None and gt_masks is not None:
            scores += [("psnr_fg", fg_psnr), ("ssim_fg", fg_ssim)]
        for name, v in scores:
            base, _, fg = name.partition("_")
            with open(vid_base + f"{base}{eval_postfix}{'_fg' if fg else ''}.txt", "a") as f:
                f.write(f"{v}\n")
    return {"psnr": psnr, "ssim": ssim_v, "psnr_fg": fg_psnr, "ssim_fg": fg_ssim}


def evaluate_in_boxes_device(rgbs, accs, bboxes, gt_imgs, gt_masks=None, bg_imgs=None, bg_indices=None):
    """evaluate_in_boxes with the frames scored on the device: the same arguments, rules and dict of lists.  rgbs is a stacked device
    tensor [N,H,W,3] (render_path(device_out=True)) or a sequence of frames; the ground truth, masks and backgrounds are uploaded
    once.  All frames of one size go into ONE hip_ops.image_metrics call with their boxes (frames of differing sizes: one call per
    size); a frame whose cropped mask is empty is skipped; the ground truth is composited as gt * mask + (1 - mask) * bg."""
    from .. import hip_ops
    out = {'psnr': [], 'ssim': [], 'fg_psnr': [], 'fg_ssim': []}
    n = len(bboxes)
    if n == 0:
        return out
    dev = _device_of(rgbs if torch.is_tensor(rgbs) else rgbs[0])
    sizes = [tuple(int(x) for x in rgbs[i].shape[:2]) for i in range(n)]
    bgs = None
    if bg_imgs is not None and gt_masks is not None:
        bgs = _on_device(bg_imgs if torch.is_tensor(bg_imgs) else np.asarray(bg_imgs), dev)
    rows = {}
    for size in dict.fromkeys(sizes):
        idx = [i for i in range(n) if sizes[i] == size]
        h, w = size
        every = len(idx) == n

        def stack(x, tail):
            if torch.is_tensor(x) or isinstance(x, np.ndarray):
                x = _on_device(x, dev)
                return (x if every else x[torch.as_tensor(idx, device=dev)]).reshape(len(idx), h, w, *tail)
            return torch.stack([_on_device(x[i], dev).reshape(h, w, *tail) for i in idx])
        pred, gt = stack(rgbs, (3,)), stack(gt_imgs, (3,))
        mask = None
        if gt_masks is not None:
            mask = stack(gt_masks, (-1,))[..., :1]
            if bgs is not None:
                bg = bgs[torch.as_tensor(np.asarray([bg_indices[i] for i in idx]), device=dev).long()]
                gt = gt * mask + (1. - mask) * bg
        boxes = np.array([[bboxes[i][0][0], bboxes[i][0][1], bboxes[i][1][0], bboxes[i][1][1]] for i in idx], dtype=np.int64)
        boxes = np.clip(boxes, 0, [w, h, w, h])
        count = np.maximum(boxes[:, 2] - boxes[:, 0], 0) * np.maximum(boxes[:, 3] - boxes[:, 1], 0) * 3.
        s = hip_ops.image_metrics(pred, gt, mask_b=mask, boxes=torch.as_tensor(boxes.astype(np.int32)).to(dev))['sums']
        for k, row, c in zip(idx, s.double().cpu().numpy(), count):
            rows[k] = (row, c)
    for i in range(n):
        row, c = rows[i]
        if gt_masks is not None and row[7] < 1:
            continue
        psnr, ssim = scores_from_sums(row[0], row[1], c, guard=False, inf_to_zero=False)
        out['psnr'].append(psnr)
        out['ssim'].append(ssim)
        if gt_masks is not None:
            psnr, ssim = scores_from_sums(row[5], row[6], row[7] * 3., guard=False, inf_to_zero=False)
            out['fg_psnr'].append(psnr)
            out['fg_ssim'].append(ssim)
    return out
