"""Times the image metrics (danbo_image_metrics, --eval_device) and the host scoring they replace (dev tool).

    python tools/bench_image_metrics.py [--steps 40] [--warmup 5] > profiles/image_metrics_measured.txt

Printed, all on the same box in the same run:
  * what tools/probe/hbm_rate.py measures (torch's streaming sum: a read rate), as the yardstick of this box;
  * the kernel pair alone (ops.image_metrics) at 512 x 512 and 1000 x 1000, N = 1 and N = 16, without masks and map, with both
    masks, with both masks and the map, through bench.py's own discipline (bench.timed: settle until two blocks agree, --warmup
    untimed calls, the median of five blocks that share --steps calls): us per call, and the achieved bytes/s against the read
    floor (24 B per pixel + 4 B per mask pixel read once, + 12 B per pixel written with the map) and against the yardstick;
  * evaluate_in_boxes / evaluate_metric (the host scoring, unchanged from the parent commit) and their _device forms on the same
    frames, from host arrays and from device tensors: ms per call, median of five calls after one;
  * run_render.py ... --eval --no_save end to end with and without --eval_device on a checkpoint trained for two steps here
    (alternating, median of five runs after one each; host clock around the whole call).
No target is set and no test asserts a speed: these are first measurements.
"""
import argparse
import contextlib
import io
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "danbo-pytorch_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

DEV = "cuda:0"


def host_timed(fn, reps=5):
    import torch
    fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return statistics.median(out), min(out), max(out)


def read_rate():
    """tools/probe/hbm_rate.py's `sum` line: torch's streaming read of 2 GiB, bytes/s"""
    import torch
    n = 1 << 29
    a = torch.empty(n, device=DEV).normal_()
    for _ in range(2):
        a.sum()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(10):
        a.sum()
    e1.record()
    torch.cuda.synchronize()
    return 4 * n / (e0.elapsed_time(e1) / 10 * 1e-3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--e2e_res", type=int, default=128, help="resolution of the end-to-end run_render comparison")
    ap.add_argument("--skip_e2e", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch
    import bench
    from core import hip_ops as ops
    from core.utils.evaluation_helpers import evaluate_in_boxes, evaluate_in_boxes_device, evaluate_metric, evaluate_metric_device
    if not torch.cuda.is_available():
        raise RuntimeError("bench_image_metrics.py measures on the GPU: none visible")
    print(f"{torch.cuda.get_device_name(0)}; torch CPU threads {torch.get_num_threads()}")
    rate = read_rate()
    print(f"yardstick: torch sum of 2 GiB reads {rate / 1e12:.2f} TB/s on this box (tools/probe/hbm_rate.py)")

    # ---- the kernel pair alone
    gen = torch.Generator(device=DEV).manual_seed(0)
    for H, W in ((512, 512), (1000, 1000)):
        for N in (1, 16):
            gt = torch.rand(N, H, W, 3, device=DEV, generator=gen)
            pred = (gt + 0.08 * torch.randn(N, H, W, 3, device=DEV, generator=gen)).clamp_(0, 1)
            ma = (torch.rand(N, H, W, device=DEV, generator=gen) < 0.5).float()
            mb = torch.rand(N, H, W, device=DEV, generator=gen)
            for name, kw, nbytes in (("no masks, no map", {}, 24), ("both masks", dict(mask_a=ma, mask_b=mb), 32),
                                     ("both masks + map", dict(mask_a=ma, mask_b=mb, want_map=True), 44)):
                sec, _, info = bench.timed(lambda kw=kw: ops.image_metrics(pred, gt, **kw), args.steps, args.warmup, None, DEV, False)
                moved = nbytes * N * H * W
                print(f"image_metrics {N:2d} x {H} x {W}, {name}: {1e6 * sec:.1f} us per call (median of {len(info['block_ms'])} blocks "
                      f"sharing {args.steps} calls, spread {100 * info['spread']:.1f} %; {len(info['settle_ms'])} settle blocks); "
                      f"{moved / 1e6:.1f} MB at the floor of {nbytes} B per pixel = {moved / sec / 1e9:.1f} GB/s = "
                      f"{100 * moved / sec / rate:.1f} % of the yardstick; {N * H * W / sec / 1e9:.2f} Gpixel/s")
            del gt, pred, ma, mb

    # ---- the scoring functions on the same frames, host and device
    rng = np.random.default_rng(0)
    for H, W in ((512, 512), (1000, 1000)):
        N = 4
        gt = rng.uniform(size=(N, H, W, 3)).astype(np.float32)
        pred = np.clip(gt + 0.08 * rng.normal(size=gt.shape), 0, 1).astype(np.float32)
        fg = (rng.uniform(size=(N, H, W, 1)) < 0.5).astype(np.float32)
        bboxes = [((W // 4, H // 8), (3 * W // 4, 7 * H // 8))] * N
        valid = [torch.arange(H * W)[::2]] * N
        d_pred, d_gt, d_fg = (torch.tensor(x, device=DEV) for x in (pred, gt, fg))
        rows = [("evaluate_in_boxes (host)", lambda: evaluate_in_boxes(pred, None, bboxes, gt, fg)),
                ("evaluate_in_boxes_device, host arrays in", lambda: evaluate_in_boxes_device(pred, None, bboxes, gt, fg)),
                ("evaluate_in_boxes_device, device tensors in", lambda: evaluate_in_boxes_device(d_pred, None, bboxes, d_gt, d_fg)),
                ("evaluate_metric eval_both (host)", lambda: evaluate_metric(pred, gt, gt_masks=fg, valid_idxs=valid, eval_both=True)),
                ("evaluate_metric_device eval_both, host arrays in",
                 lambda: evaluate_metric_device(pred, gt, gt_masks=fg, valid_idxs=valid, eval_both=True)),
                ("evaluate_metric_device eval_both, device tensors in",
                 lambda: evaluate_metric_device(d_pred, d_gt, gt_masks=d_fg, valid_idxs=valid, eval_both=True))]
        for name, fn in rows:
            med, lo, hi = host_timed(fn)
            print(f"{N} x {H} x {W} {name}: {1e3 * med:.2f} ms per call = {1e3 * med / N:.2f} ms per frame (median of 5 calls, "
                  f"{1e3 * lo:.2f} .. {1e3 * hi:.2f} ms)")

    # ---- run_render end to end
    if args.skip_e2e:
        return
    import run_nerf
    import run_render
    with tempfile.TemporaryDirectory() as tmp:
        cfg = os.path.join(ROOT, "danbo-pytorch_amd", "configs", "surreal", "danbo_fast.txt")
        res = str(args.e2e_res)
        quiet = lambda: contextlib.redirect_stdout(io.StringIO())      # noqa: E731  (the entry points print their set-up)
        with quiet():
            run_nerf.train(["--config", cfg, "--basedir", tmp, "--expname", "demo", "--syn_poses", "2", "--syn_cams", "2",
                            "--syn_res", res, "--syn_rest_scale", "0.714", "--N_rand", "512", "--N_sample_images", "4",
                            "--i_print", "1000", "--i_weights", "2", "--i_testset", "1000", "--render_factor", "0", "--n_iters", "2"])
        base = ["--nerf_args", os.path.join(tmp, "demo", "args.txt"), "--ckptpath", os.path.join(tmp, "demo", "000002.tar"),
                "--dataset", "synthetic", "--entry", "val", "--outputdir", os.path.join(tmp, "out"), "--render_type", "val",
                "--render_res", res, res, "--eval", "--no_save", "--runname", "r"]
        times = {"host": [], "device": []}
        for i in range(6):
            for name, extra in (("host", []), ("device", ["--eval_device"])):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                with quiet():
                    out = run_render.run_render(base + extra)
                torch.cuda.synchronize()
                if i:
                    times[name].append(time.perf_counter() - t0)
        n = len(out[3]["psnr"])
        for name, t in times.items():
            print(f"run_render --render_type val --eval --no_save at {res} x {res}, {n} scored frames, scoring on the {name}: "
                  f"{1e3 * statistics.median(t):.1f} ms per run (median of 5 after one, {1e3 * min(t):.1f} .. {1e3 * max(t):.1f} ms; "
                  f"model load and data set-up included in both)")


if __name__ == "__main__":
    main()
