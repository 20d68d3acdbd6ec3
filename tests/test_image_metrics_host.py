"""Image metrics (danbo_image_metrics, --eval_device), the part that needs no GPU: the serial restatement of csrc/metrics_math.hpp
against the golden SSIM vector and a float64 evaluation, its box semantics, the host arithmetic of scores_from_sums, the argument
checks (which return before any launch) and the new flags.  The binding of include/danbo_metrics.h: tests/test_abi_binding.py."""
import numpy as np
import pytest
import torch

import metrics_ref as ref
from helpers import ADDR as P, EINVAL, golden, hip_lib as _lib     # P: an address no check follows


# ----------------------------------------------------------------------------- the serial restatement
def test_serial_map_against_the_golden():
    g = golden("ssim_known_answer")
    pred, gt = (np.ascontiguousarray(g[k].transpose(0, 2, 3, 1)) for k in ("pred", "gt"))
    _, m = ref.host_metrics(pred, gt)
    m = m.transpose(0, 3, 1, 2)
    e_same, e_valid = np.abs(m - g["map_same"]).max(), np.abs(m[:, :, 5:-5, 5:-5] - g["map_valid"]).max()
    e_one = float(np.abs(m[0, :, :4, :] - 1.0).max())
    print(f"map_same {e_same:.3e}  map_valid {e_valid:.3e}  error-free rows {e_one:.3e}")
    assert m.shape == g["map_same"].shape and e_same < ref.MAP_TOL and e_valid < ref.MAP_TOL
    assert e_one < 1e-5


@pytest.fixture(scope="module")
def textured():
    """3 x 37 x 53 frames, both masks, computed once: (inputs, serial sums and map, float64 sums and map)"""
    N, H, W = 3, 37, 53
    pred, gt = ref.frames(11, N, H, W)
    rng = np.random.default_rng(12)
    ma = (rng.uniform(size=(N, H, W)) < 0.6).astype(np.float32)
    mb = rng.uniform(size=(N, H, W)).astype(np.float32)           # fractional weights
    sums, m = ref.host_metrics(pred, gt, ma, mb)
    sums64, m64 = ref.metrics_f64(pred, gt, ma, mb)
    return dict(pred=pred, gt=gt, ma=ma, mb=mb, sums=sums, map=m, sums64=sums64, map64=m64)


def test_serial_sums_against_float64(textured):
    t = textured
    s, d = t["sums"].astype(np.float64), t["sums64"]
    N, H, W = t["ma"].shape
    assert np.abs(t["map"] - t["map64"]).max() < ref.MAP_TOL
    for se, ss, cnt, cnt64 in ((0, 1, np.full(N, H * W * 3.), np.full(N, H * W * 3.)), (2, 3, 3 * s[:, 4], 3 * d[:, 4]),
                               (5, 6, 3 * s[:, 7], 3 * d[:, 7])):
        e_ssim = np.abs(s[:, ss] / cnt - d[:, ss] / cnt64).max()
        e_psnr = np.abs(ref.psnr(s[:, se], cnt) - ref.psnr(d[:, se], cnt64)).max()
        print(f"slots {se},{ss}: ssim mean {e_ssim:.3e}  psnr {e_psnr:.3e} dB")
        assert e_ssim < ref.SSIM_TOL and e_psnr < ref.PSNR_TOL
    assert np.array_equal(s[:, 4], t["ma"].reshape(N, -1).sum(-1))             # 0 / 1 weights: the count, exactly
    assert np.abs(s[:, 7] - d[:, 7]).max() < 1e-6 * d[:, 7].max()


def test_serial_null_masks_and_constant_offset():
    pred, gt = ref.frames(3, 2, 20, 33)
    sums, _ = ref.host_metrics(pred, gt, want_map=False)
    assert np.array_equal(sums[:, 2:].view(np.uint32), np.zeros((2, 6), np.uint32))            # +0, not -0
    sums, _ = ref.host_metrics(np.full((1, 24, 20, 3), 0.5, np.float32), np.full((1, 24, 20, 3), 0.6, np.float32), want_map=False)
    assert abs(ref.psnr(float(sums[0, 0]), 24 * 20 * 3) - 20.0) < 1e-3


BOXES = {"two_borders": (0, 0, 19, 14), "inside": (7, 5, 30, 29), "one_pixel": (12, 9, 13, 10), "over_reaching": (40, 30, 90, 70),
         "negative_corner": (-5, -3, 9, 8)}


@pytest.mark.parametrize("name", sorted(BOXES))
def test_serial_box_is_the_crop(name, textured):
    """the map (and the sums up to the tree's order) of a box = those of the cropped arrays under the whole-image box"""
    t = textured
    N, H, W = t["ma"].shape
    box = BOXES[name]
    x0, y0, x1, y1 = ref.clamp_box(box, H, W)
    boxes = np.tile(np.array(box, np.int32), (N, 1))
    sums, m = ref.host_metrics(t["pred"], t["gt"], t["ma"], t["mb"], boxes=boxes)
    crop = lambda a: np.ascontiguousarray(a[:, y0:y1, x0:x1])      # noqa: E731
    c_sums, c_map = ref.host_metrics(crop(t["pred"]), crop(t["gt"]), crop(t["ma"]), crop(t["mb"]))
    assert np.array_equal(m[:, y0:y1, x0:x1].view(np.uint32), c_map.view(np.uint32))
    outside = np.ones((N, H, W), bool)
    outside[:, y0:y1, x0:x1] = False
    assert np.all(m[outside] == ref.MAP_FILL)                        # pixels outside the box are not touched
    # the same non-negative values through two trees of at most 22 levels, each level one rounding of 2^-24
    assert np.allclose(sums, c_sums, rtol=2 * 22 * 2.0 ** -24, atol=0)


def test_serial_empty_box(textured):
    t = textured
    N = len(t["pred"])
    boxes = np.array([[5, 5, 5, 20], [9, 30, 20, 12], [60, 2, 70, 9]], np.int32)               # no width; y1 < y0; outside the image
    sums, m = ref.host_metrics(t["pred"], t["gt"], t["ma"], t["mb"], boxes=boxes)
    assert np.array_equal(sums.view(np.uint32), np.zeros((N, 8), np.uint32))
    assert np.all(m == ref.MAP_FILL)


# ----------------------------------------------------------------------------- scores_from_sums
def test_scores_from_sums():
    from core.utils.evaluation_helpers import _masked_scores, scores_from_sums
    assert scores_from_sums([0.], [30.], [30.]) == (0.0, 1.0)                         # zero error: inf -> 0
    assert scores_from_sums([0., 3.], [0., 150.], [0., 300.]) == (10.0, 0.25)         # an empty mask: max(denominator, 1)
    psnr, ssim = scores_from_sums([0.], [0.], [0.], guard=False, inf_to_zero=False, mean=False)
    assert np.isnan(psnr[0]) and np.isnan(ssim[0])
    rng = np.random.default_rng(5)
    se, ss = rng.uniform(size=(3, 6, 5, 3)), rng.uniform(size=(3, 6, 5, 3))
    mask = (rng.uniform(size=(3, 6, 5, 1)) < 0.5).astype(np.float64)
    mask[2] = 0
    want = _masked_scores(se, ss, mask)
    got = scores_from_sums((se * mask).reshape(3, -1).sum(-1), (ss * mask).reshape(3, -1).sum(-1), mask.reshape(3, -1).sum(-1) * 3.)
    assert np.allclose(got, want, rtol=1e-12)
    # evaluate_in_boxes' arithmetic: -10 log10(se.mean()), s.mean(); (se * mask).sum() / (mask.sum() * 3)
    psnr, ssim = scores_from_sums(se[0].sum(), ss[0].sum(), se[0].size, guard=False, inf_to_zero=False)
    assert abs(psnr - -10. * np.log10(se[0].mean())) < 1e-12 and abs(ssim - ss[0].mean()) < 1e-12
    psnr, ssim = scores_from_sums((se[0] * mask[0]).sum(), (ss[0] * mask[0]).sum(), mask[0].sum() * 3., guard=False, inf_to_zero=False)
    assert abs(psnr - -10. * np.log10((se[0] * mask[0]).sum() / (mask[0].sum() * 3.))) < 1e-12


# ----------------------------------------------------------------------------- argument checks
def image_metrics(pred=P, gt=P, mask_a=None, mask_b=None, boxes=None, n=2, h=20, w=24, window=P, win=11, ws=P, sums=P, ssim=P):
    return _lib().danbo_image_metrics(pred, gt, mask_a, mask_b, boxes, n, h, w, window, win, ws, sums, ssim, None)


@pytest.mark.parametrize("kw", [dict(pred=None), dict(gt=None), dict(window=None), dict(ws=None), dict(sums=None), dict(n=-1),
                                dict(h=0), dict(h=4097), dict(w=0), dict(w=4097), dict(h=-3), dict(win=10), dict(win=0), dict(win=-1),
                                dict(win=17), dict(win=2), dict(pred=P + 4), dict(gt=P + 8), dict(ssim=P + 4), dict(ws=P + 2)])
def test_image_metrics_rejects_before_any_launch(kw):
    assert image_metrics(**kw) == EINVAL


def test_image_metrics_of_no_images_launches_nothing():
    assert image_metrics(n=0) == 0
    assert image_metrics(n=0, ssim=None, win=1) == 0


def test_workspace_bytes():
    lib, r = _lib(), ref.host_lib()
    for size in ((1, 0, 8), (1, 8, 0), (1, 4097, 8), (1, 8, 4097), (-1, 8, 8), (1, -8, 8)):
        assert lib.danbo_image_metrics_workspace_bytes(*size) == 0 == r.ref_metrics_workspace_bytes(*size), size
    for size in ((1, 1, 1), (3, 37, 53), (16, 1000, 1000), (1, 4096, 4096), (0, 16, 32), (2, 16, 32), (2, 17, 33)):
        n = lib.danbo_image_metrics_workspace_bytes(*size)
        assert n > 0 and n % 4 == 0 and n == r.ref_metrics_workspace_bytes(*size), size


def test_wrapper_raises_on_cpu_tensors():
    from core import hip_ops as ops
    from core.utils.evaluation_helpers import _gauss
    x = torch.zeros(1, 8, 8, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.image_metrics(x, x)
    assert ops.METRICS_WIN == _gauss().numel() == 11


def test_both_parsers_know_eval_device():
    import run_render
    from core.config import config_parser
    base = ["--nerf_args", "a", "--ckptpath", "c", "--dataset", "synthetic", "--entry", "val", "--runname", "r"]
    p = run_render.config_parser()
    assert p.parse_args(base).eval_device is False
    a = p.parse_args(base + ["--eval", "--eval_device", "--no_save"])
    assert a.eval and a.eval_device and a.no_save
    assert config_parser().parse_args([]).eval_device is False
    assert config_parser().parse_args(["--eval_device"]).eval_device is True
