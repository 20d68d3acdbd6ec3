"""GPU tests of the image metrics (danbo_image_metrics, csrc/k_metrics.hip): the kernel against the serial restatement of
csrc/metrics_math.hpp bit for bit at the shapes where tile, halo and tree logic can go wrong, guard words, determinism, a side
stream, the golden known answer through the wrapper; evaluate_metric_device / evaluate_in_boxes_device against a float64 evaluation
(and the CPU functions against the same, which shows the inputs are fair); run_render --eval_device and validate end to end."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import metrics_ref as ref
from helpers import ROOT, golden
from mesh_ref import GUARD, N_GUARD

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TH, TW = 16, 32


def T(x, dtype=torch.float32):
    return None if x is None else torch.tensor(np.ascontiguousarray(x), dtype=dtype, device=DEV)


def guarded(n, fill):
    """-> (whole uint32 device buffer with N_GUARD guard words on either side, the float32 view of the n payload words);
    the payload starts 64 bytes into a torch allocation: 16-byte aligned"""
    buf = torch.full((n + 2 * N_GUARD,), GUARD, dtype=torch.int32, device=DEV)
    pay = buf[N_GUARD:N_GUARD + n].view(torch.float32)
    pay.fill_(fill)
    return buf, pay


def guards_intact(buf):
    return bool((buf[:N_GUARD] == GUARD).all() and (buf[-N_GUARD:] == GUARD).all())


def gpu_metrics(pred, gt, ma=None, mb=None, boxes=None, win=11, want_map=True, stream=None, w=None):
    """danbo_image_metrics through the C ABI on guarded buffers -> sums [N,8], map [N,H,W,3] (pre-filled with MAP_FILL) as numpy;
    the workspace starts as NaNs"""
    from core import _hip
    from core._hip import ptr
    lib = _hip.lib()
    N, H, W = pred.shape[:3]
    d_pred, d_gt, d_ma, d_mb = T(pred), T(gt), T(ma), T(mb)
    d_box = T(boxes, torch.int32)
    d_w = T(ref.window(win) if w is None else w)
    n_bytes = lib.danbo_image_metrics_workspace_bytes(N, H, W)
    assert n_bytes > 0 and n_bytes % 4 == 0
    ws_buf, ws = guarded(n_bytes // 4, float("nan"))
    s_buf, sums = guarded(N * 8, float("nan"))
    m_buf, m = guarded(N * H * W * 3, float(ref.MAP_FILL)) if want_map else (None, None)
    st = torch.cuda.current_stream() if stream is None else stream
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    rc = lib.danbo_image_metrics(ptr(d_pred), ptr(d_gt), ptr(d_ma), ptr(d_mb), ptr(d_box), N, H, W, ptr(d_w), win, ptr(ws), ptr(sums),
                                 ptr(m), st.cuda_stream)
    assert rc == 0, rc
    st.synchronize()
    assert guards_intact(ws_buf) and guards_intact(s_buf) and (m_buf is None or guards_intact(m_buf)), "a guard word was overwritten"
    return sums.cpu().numpy().reshape(N, 8), (m.cpu().numpy().reshape(N, H, W, 3) if want_map else None)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def masks(seed, N, H, W):
    rng = np.random.default_rng(seed)
    return (rng.uniform(size=(N, H, W)) < 0.6).astype(np.float32), rng.uniform(size=(N, H, W)).astype(np.float32)


def check_bits(pred, gt, ma=None, mb=None, boxes=None, win=11, w=None):
    want_s, want_m = ref.host_metrics(pred, gt, ma, mb, boxes, win=win, w=w)
    got_s, got_m = gpu_metrics(pred, gt, ma, mb, boxes, win=win, w=w)
    assert same_bits(got_m, want_m), f"map: {int((got_m.view(np.uint32) != want_m.view(np.uint32)).sum())} words differ"
    assert same_bits(got_s, want_s), (got_s, want_s)
    return got_s, got_m


SHAPES = [(1, 1, 1), (2, 3, 7), (1, TH - 1, TW - 1), (1, TH, TW), (2, TH + 1, TW + 1), (1, TH - 1, TW + 1), (1, TH + 1, TW - 1),
          (1, 2 * TH, 2 * TW), (1, 2 * TH + 1, 3 * TW + 1)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_equals_the_serial_restatement(shape):
    N, H, W = shape
    pred, gt = ref.frames(H * 100 + W, N, H, W)
    check_bits(pred, gt, *masks(H + W, N, H, W))


@pytest.fixture(scope="module")
def scene():
    N, H, W = 3, 37, 53
    pred, gt = ref.frames(11, N, H, W)
    ma, mb = masks(12, N, H, W)
    return pred, gt, ma, mb


def test_boxes_inside_a_tile_across_four_tiles_and_clamped(scene):
    pred, gt, ma, mb = scene
    boxes = np.array([[3, 2, 20, 12], [20, 10, 45, 30], [40, 30, 90, 70]], np.int32)
    s, m = check_bits(pred, gt, ma, mb, boxes)
    for n, b in enumerate(boxes):                                   # map pixels outside the box are untouched
        x0, y0, x1, y1 = ref.clamp_box(b, 37, 53)
        out = np.ones((37, 53), bool)
        out[y0:y1, x0:x1] = False
        assert np.all(m[n][out] == ref.MAP_FILL) and np.all(m[n][~out] != ref.MAP_FILL)
    assert (s[:, 0] > 0).all()


def test_empty_and_negative_boxes(scene):
    pred, gt, ma, mb = scene
    boxes = np.array([[5, 5, 5, 20], [9, 30, 20, 12], [-4, -2, 6, 9]], np.int32)
    s, m = check_bits(pred, gt, ma, mb, boxes)
    assert same_bits(s[:2], np.zeros((2, 8), np.float32)) and np.all(m[:2] == ref.MAP_FILL)


@pytest.mark.parametrize("which", ["fractional_both", "a_only", "b_only", "neither"])
def test_mask_combinations(scene, which):
    pred, gt, ma, mb = scene
    a = {"fractional_both": mb, "a_only": ma, "b_only": None, "neither": None}[which]
    b = {"fractional_both": ma * mb, "a_only": None, "b_only": mb, "neither": None}[which]
    s, _ = check_bits(pred, gt, a, b)
    if a is None:
        assert same_bits(s[:, 2:5], np.zeros((3, 3), np.float32))
    if b is None:
        assert same_bits(s[:, 5:8], np.zeros((3, 3), np.float32))


@pytest.mark.parametrize("win", [1, 11, 15])
def test_window_sizes(scene, win):
    pred, gt, ma, mb = scene
    check_bits(pred[:1], gt[:1], ma[:1], mb[:1], np.array([[2, 1, 50, 36]], np.int32), win=win)


def test_flat_image_pair():
    """the variance cancels: only bit-equality says anything here"""
    pred, gt = np.full((1, 21, 40, 3), 0.7, np.float32), np.full((1, 21, 40, 3), 0.7, np.float32)
    gt[0, 10:, :, 1] = 0.25
    pred[0, :, 20:] = 0.3
    check_bits(pred, gt, *masks(3, 1, 21, 40))


def test_more_tiles_than_lanes():
    """552 tiles, 1024 leaves: the image's tree has levels wider than the reducing workgroup (a 3-tap window keeps the serial
    side quick; the tiling and the trees do not depend on the window)"""
    pred, gt = ref.frames(5, 1, 23 * TH - 3, 24 * TW - 5)
    ma, _ = masks(6, 1, 23 * TH - 3, 24 * TW - 5)
    check_bits(pred, gt, ma, None, win=3, w=np.array([0.25, 0.5, 0.25], np.float32))


def test_two_calls_and_a_side_stream_give_the_same_bits(scene):
    pred, gt, ma, mb = scene
    boxes = np.array([[3, 2, 20, 12], [20, 10, 45, 30], [0, 0, 53, 37]], np.int32)
    s0, m0 = gpu_metrics(pred, gt, ma, mb, boxes)
    s1, m1 = gpu_metrics(pred, gt, ma, mb, boxes)
    s2, m2 = gpu_metrics(pred, gt, ma, mb, boxes, stream=torch.cuda.Stream())
    assert same_bits(s0, s1) and same_bits(m0, m1) and same_bits(s0, s2) and same_bits(m0, m2)


def test_golden_known_answer_through_the_wrapper():
    from core import hip_ops as ops
    g = golden("ssim_known_answer")
    pred, gt = (T(g[k].transpose(0, 2, 3, 1)) for k in ("pred", "gt"))
    out = ops.image_metrics(pred, gt, want_map=True)
    m = out["ssim_map"].cpu().numpy().transpose(0, 3, 1, 2)
    e_same, e_valid = np.abs(m - g["map_same"]).max(), np.abs(m[:, :, 5:-5, 5:-5] - g["map_valid"]).max()
    print(f"map_same {e_same:.3e}  map_valid {e_valid:.3e}")
    assert e_same < ref.MAP_TOL and e_valid < ref.MAP_TOL
    assert float(np.abs(m[0, :, :4, :] - 1.0).max()) < 1e-5
    s = out["sums"].double().cpu().numpy()
    assert tuple(s.shape) == (2, 8) and np.abs(s[:, 1] / m[0].size - g["map_same"].reshape(2, -1).mean(-1)).max() < ref.SSIM_TOL
    assert ops.image_metrics(pred, gt)["ssim_map"] is None
    boxes = T([[2, 3, 20, 25], [0, 0, 24, 28]], torch.int32)
    boxed = ops.image_metrics(pred, gt, boxes=boxes, want_map=True)["ssim_map"]
    assert float(boxed[0, :3].abs().max()) == 0.0 and torch.equal(boxed[1], out["ssim_map"][1])     # 0 outside the box


# ----------------------------------------------------------------------------- the scoring functions end to end
def _metric_f64(rgbs, gt, fg=None, valid=None, render_factor=0):
    """evaluate_metric in float64 -> its result dictionary"""
    rgbs, gt = np.asarray(rgbs, np.float64), np.asarray(gt, np.float64)
    if fg is not None:
        keep = np.where(fg.reshape(len(fg), -1).sum(-1) > 0)[0]
        rgbs, gt, fg = rgbs[keep], gt[keep], fg[keep]
        valid = valid[keep] if valid is not None else None
    if render_factor > 0:
        rgbs = F.interpolate(torch.tensor(rgbs).permute(0, 3, 1, 2), size=gt.shape[1:3], mode="bilinear",
                             align_corners=False).permute(0, 2, 3, 1).numpy()
    s, _ = ref.metrics_f64(rgbs, gt, valid, fg)
    n, (H, W) = len(gt), gt.shape[1:3]

    def scores(se, ss, denom):
        with np.errstate(divide="ignore"):
            p = -10. * np.log10(se / np.maximum(denom, 1.))
        p[p == np.inf] = 0.
        return float(p.mean()), float((ss / np.maximum(denom, 1.)).mean())
    fg_p = fg_s = None
    if fg is not None:
        fg_p, fg_s = scores(s[:, 5], s[:, 6], 3. * s[:, 7])
    if valid is not None:
        p, v = scores(s[:, 2], s[:, 3], 3. * s[:, 4])
    elif fg is not None:
        p, v = fg_p, fg_s
    else:
        p, v = scores(s[:, 0], s[:, 1], np.full(n, H * W * 3.))
    return {"psnr": p, "ssim": v, "psnr_fg": fg_p, "ssim_fg": fg_s}


def _close(got, want):
    for k in ("psnr", "ssim", "psnr_fg", "ssim_fg"):
        if want[k] is None:
            assert got[k] is None, k
            continue
        print(f"{k}: {got[k]!r} against {want[k]!r}: {abs(got[k] - want[k]):.3e}")
        assert abs(got[k] - want[k]) < (ref.PSNR_TOL if k.startswith("psnr") else ref.SSIM_TOL), (k, got[k], want[k])


@pytest.mark.parametrize("case", ["no_masks", "foreground", "eval_both", "no_person", "render_factor", "device_inputs"])
def test_evaluate_metric_device(case, tmp_path):
    from core.utils.evaluation_helpers import evaluate_metric, evaluate_metric_device
    N, H, W = 3, 24, 20
    pred, gt = ref.frames(21, N, H, W)
    rng = np.random.default_rng(22)
    fg = (rng.uniform(size=(N, H, W, 1)) < 0.5).astype(np.float32)
    valid_idxs = [torch.tensor(np.sort(rng.choice(H * W, size=k, replace=False))) for k in (200, 333, 480)]
    valid = np.zeros((N, H * W), np.float32)
    for i, idx in enumerate(valid_idxs):
        valid[i, idx.numpy()] = 1
    valid = valid.reshape(N, H, W)
    kw, f64 = {}, dict(rgbs=pred, gt=gt)
    if case in ("foreground", "device_inputs"):
        kw, f64 = dict(gt_masks=fg), dict(f64, fg=fg)
    elif case in ("eval_both", "no_person"):
        if case == "no_person":
            fg[1] = 0
        kw, f64 = dict(gt_masks=fg, valid_idxs=valid_idxs, eval_both=True), dict(f64, fg=fg, valid=valid)
    elif case == "render_factor":
        small, _ = ref.frames(23, N, H // 2, W // 2)
        pred = small
        kw, f64 = dict(render_factor=2), dict(rgbs=small, gt=gt, render_factor=2)
    want = _metric_f64(**f64)
    cpu = evaluate_metric(pred, gt, vid_base=str(tmp_path / "cpu_"), eval_postfix="_x", **kw)
    if case == "device_inputs":
        kw = dict(gt_masks=T(fg))
        dev = evaluate_metric_device(T(pred), T(gt), vid_base=str(tmp_path / "dev_"), eval_postfix="_x", **kw)
    else:
        dev = evaluate_metric_device(pred, gt, vid_base=str(tmp_path / "dev_"), eval_postfix="_x", **kw)
    _close(cpu, want)                                   # the inputs are fair: the existing CPU path meets the bounds
    _close(dev, want)
    assert {k for k, v in dev.items() if v is None} == {k for k, v in cpu.items() if v is None}
    files = sorted(f[4:] for f in os.listdir(tmp_path) if f.startswith("cpu_"))
    assert files and files == sorted(f[4:] for f in os.listdir(tmp_path) if f.startswith("dev_"))
    for f in files:
        assert len(open(tmp_path / ("cpu_" + f)).readlines()) == len(open(tmp_path / ("dev_" + f)).readlines()) == 1


def test_evaluate_metric_device_zero_error_is_zero():
    from core.utils.evaluation_helpers import evaluate_metric, evaluate_metric_device
    _, gt = ref.frames(31, 2, 24, 20)
    fg = np.ones((2, 24, 20, 1), np.float32)
    cpu, dev = evaluate_metric(gt, gt, gt_masks=fg), evaluate_metric_device(gt, gt, gt_masks=fg)
    assert cpu["psnr"] == dev["psnr"] == 0.0 and cpu["psnr_fg"] == dev["psnr_fg"] == 0.0        # inf -> 0, the reference's convention
    assert abs(dev["ssim"] - 1.0) < 1e-5


@pytest.mark.parametrize("with_bg", [False, True])
def test_evaluate_in_boxes_device(with_bg):
    from core.utils.evaluation_helpers import evaluate_in_boxes, evaluate_in_boxes_device
    N, H, W = 3, 40, 36
    pred, gt = ref.frames(41, N, H, W)
    rng = np.random.default_rng(42)
    fg = (rng.uniform(size=(N, H, W, 1)) < 0.5).astype(np.float32)
    bboxes = [(np.array([4, 6]), np.array([30, 38])), (np.array([0, 0]), np.array([17, 15])), (np.array([10, 3]), np.array([36, 40]))]
    fg[1, :15, :17] = 0                                              # frame 1: its cropped mask is empty -> skipped
    bgs = rng.uniform(size=(2, H, W, 3)).astype(np.float32)
    extra = dict(bg_imgs=bgs, bg_indices=np.array([1, 0, 1])) if with_bg else {}
    cpu = evaluate_in_boxes(pred, None, bboxes, gt.reshape(N, -1), fg, **extra)
    dev = evaluate_in_boxes_device(T(pred), None, bboxes, gt.reshape(N, -1), fg, **extra)
    want = {k: [] for k in cpu}
    for i in (0, 2):
        (x0, y0), (x1, y1) = bboxes[i]
        g = gt[i].astype(np.float64)
        if with_bg:
            g = g * fg[i] + (1. - fg[i]) * bgs[extra["bg_indices"][i]]
        r, g, m = pred[i, y0:y1, x0:x1].astype(np.float64), g[y0:y1, x0:x1], fg[i, y0:y1, x0:x1].astype(np.float64)
        s, se = ref.ssim_f64(r, g), np.square(g - r)
        want["psnr"].append(-10. * np.log10(se.mean()))
        want["ssim"].append(s.mean())
        want["fg_psnr"].append(-10. * np.log10((se * m).sum() / (3. * m.sum())))
        want["fg_ssim"].append((s * m).sum() / (3. * m.sum()))
    for got in (cpu, dev):
        assert sorted(got) == sorted(want)
        for k in want:
            assert len(got[k]) == 2, (k, got[k])                     # the skipped frame is skipped
            tol = ref.PSNR_TOL if "psnr" in k else ref.SSIM_TOL
            print(k, np.abs(np.array(got[k]) - np.array(want[k])).max())
            assert np.abs(np.array(got[k]) - np.array(want[k])).max() < tol, (k, got[k], want[k])
    # no masks at all: two lists stay empty, as on the host
    cpu, dev = evaluate_in_boxes(pred, None, bboxes, gt), evaluate_in_boxes_device(pred, None, bboxes, gt)
    assert len(dev["psnr"]) == len(cpu["psnr"]) == 3 and dev["fg_psnr"] == cpu["fg_psnr"] == []
    assert np.abs(np.array(dev["psnr"]) - np.array(cpu["psnr"])).max() < 2 * ref.PSNR_TOL


def test_evaluate_in_boxes_device_frames_of_two_sizes():
    from core.utils.evaluation_helpers import evaluate_in_boxes, evaluate_in_boxes_device
    a, ga = ref.frames(51, 2, 20, 24)
    b, gb = ref.frames(52, 1, 18, 30)
    rgbs, gts = [a[0], b[0], a[1]], [ga[0], gb[0], ga[1]]
    bboxes = [((2, 3), (20, 18)), ((0, 0), (30, 18)), ((5, 1), (24, 20))]
    cpu = evaluate_in_boxes(rgbs, None, bboxes, gts)
    dev = evaluate_in_boxes_device([T(x) for x in rgbs], None, bboxes, gts)
    assert np.abs(np.array(dev["psnr"]) - np.array(cpu["psnr"])).max() < 2 * ref.PSNR_TOL
    assert np.abs(np.array(dev["ssim"]) - np.array(cpu["ssim"])).max() < 2 * ref.SSIM_TOL


# ----------------------------------------------------------------------------- entry points
def test_run_render_eval_device_and_validate(tmp_path):
    """a two-step training run writes the checkpoint; run_render scores the validation frames on the host and on the device, and
    validate (the training loop's validation pass) does both on the same caster"""
    import run_nerf
    import run_render
    from core.load_data import load_data
    cfg = os.path.join(ROOT, "danbo-pytorch_amd", "configs", "surreal", "danbo_fast.txt")
    trainer = run_nerf.train(["--config", cfg, "--basedir", str(tmp_path), "--expname", "demo", "--syn_poses", "2", "--syn_cams", "2",
                              "--syn_res", "32", "--syn_rest_scale", "0.714", "--N_rand", "512", "--N_sample_images", "4",
                              "--i_print", "1000", "--i_weights", "2", "--i_testset", "1000", "--render_factor", "0", "--n_iters", "2"])
    log = tmp_path / "demo"
    base = ["--nerf_args", str(log / "args.txt"), "--ckptpath", str(log / "000002.tar"), "--dataset", "synthetic", "--entry", "val",
            "--outputdir", str(tmp_path / "out"), "--render_type", "val", "--render_res", "32", "32", "--eval", "--no_save"]
    rgbs, _, _, host = run_render.run_render(base + ["--runname", "host"])
    d_rgbs, d_accs, _, dev = run_render.run_render(base + ["--runname", "dev", "--eval_device"])
    assert torch.is_tensor(d_rgbs) and d_rgbs.is_cuda and d_accs.is_cuda and tuple(d_rgbs.shape) == rgbs.shape
    assert sorted(dev) == sorted(host)
    for k in host:
        assert len(dev[k]) == len(host[k]) > 0
        e = np.abs(np.array(dev[k]) - np.array(host[k])).max()
        print(f"run_render {k}: {e:.3e}")
        assert e < (ref.PSNR_TOL if "psnr" in k else ref.SSIM_TOL), (k, dev[k], host[k])
    for run in ("host", "dev"):
        assert (tmp_path / "out" / run / "score_final.txt").exists() and (tmp_path / "out" / run / "scores.npy").exists()
        assert not (tmp_path / "out" / run / "image.npy").exists()
    assert len(open(tmp_path / "out" / "dev" / "score_final.txt").readlines()) == len(open(tmp_path / "out" / "host" / "score_final.txt").readlines())

    _, render_data, _ = load_data(trainer.args, device=torch.device(DEV))
    args_dev = copy.copy(trainer.args)
    args_dev.eval_device = True
    m_host, _, _ = run_nerf.validate(trainer.args, render_data, trainer.render_kwargs_test, torch.device(DEV), str(tmp_path / "vh_"))
    for _ in range(2):                                  # the second pass scores against the ground truth kept on the device
        m_dev, r_dev, _ = run_nerf.validate(args_dev, render_data, trainer.render_kwargs_test, torch.device(DEV), str(tmp_path / "vd_"))
        assert r_dev.is_cuda and sorted(m_dev) == ["psnr", "psnr_fg", "ssim", "ssim_fg"]
        for k in m_dev:
            print(f"validate {k}: {m_dev[k]!r} against {m_host[k]!r}")
            assert m_dev[k] is not None and abs(m_dev[k] - m_host[k]) < (ref.PSNR_TOL if "psnr" in k else ref.SSIM_TOL)
    assert "_eval_device" in render_data
    assert len(open(str(tmp_path / "vd_") + "psnr.txt").readlines()) == 2 == 2 * len(open(str(tmp_path / "vh_") + "psnr.txt").readlines())
