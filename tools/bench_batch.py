"""Times a training batch on the host path and on the device path, and the training loop on either (dev tool).

    python tools/bench_batch.py [--images 64] [--res 512] [--iters 300] > profiles/batch_measured.txt

Printed, all on the same box in the same run, at the workload's batch (16 images x 192 rays, configs/perfcap/danbo_fast.txt) drawn
from --images images of --res x --res pixels (random colours and masks: a batch costs the same whatever the pixels hold):
  (a) the host path as the parent commit has it: PoseImageDataset.sample_batch in numpy and the trainer's one .to(device) per tensor;
      host milliseconds per batch, the clock stopped after a device synchronise;
  (b) the device path, sample_batch(on_device=True): the draw alone, then draw + staging copy + launch (host clock, synchronised
      like (a)), and danbo_batch_gather's own time by device events around back-to-back launches on a fixed draw, with the bytes it
      moves per second;
  (c) run_nerf.py's loop on that data set with and without --device_data, the two alternating: seconds per iteration between the
      first --warm iterations and the last, both marks after a device synchronise.  The loop is run_nerf.train itself; only its
      data set is built here (the teacher render of 64 images of 512 x 512 is not what is measured).
(a) and (b): the median of five blocks of --steps batches after --warmup batches, with the blocks' range.
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
for p in (ROOT, os.path.join(ROOT, "danbo-pytorch_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

DEV = "cuda:0"
N_IMAGES, N_RAND = 16, 3072


def arrays(n_images, res, n_cams=4):
    """-> (synthetic_arrays, (imgs, fgs)) of n_images images: seeded poses and cameras, random colours, masks of 0 / 0.25 / 1"""
    import numpy as np
    from core.load_data import synthetic_arrays
    arr = synthetic_arrays(n_poses=n_images // n_cams, n_cams=n_cams, H=res, W=res)
    rng = np.random.default_rng(0)
    imgs = rng.random((n_images, res, res, 3), dtype=np.float32)
    fgs = rng.choice(np.array([0, 0.25, 1], np.float32), size=(n_images, res, res, 1))
    return arr, (imgs, fgs)


def dataset(arr, images, **flags):
    import numpy as np
    from core.load_data import PoseImageDataset
    imgs, fgs = images
    n, res = imgs.shape[:2]
    return PoseImageDataset(imgs, fgs, np.ones((1, res, res, 3), np.float32), np.zeros(n, np.int64), arr["c2ws"], arr["focals"], arr["kp3d"],
                            arr["bones"], arr["skts"], arr["rest_pose"], cam_idxs=arr["cam_idxs"], **flags)


def blocks(fn, steps, warmup, sync):
    """median, min, max over five blocks of the seconds one call of fn takes (host clock; sync() before either reading)"""
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(5):
        sync()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        sync()
        out.append((time.perf_counter() - t0) / steps)
    return statistics.median(out), min(out), max(out)


def ms(t):
    return f"{1e3 * t[0]:.3f} ms (five blocks: {1e3 * t[1]:.3f} .. {1e3 * t[2]:.3f} ms)"


def kernel_time(ds, steps, warmup):
    """danbo_batch_gather alone on one fixed draw: device events around `steps` back-to-back launches -> seconds per launch"""
    import numpy as np
    import torch
    from core import _hip
    import batch_ref as ref
    per, picks, pixels, noise = ref.draw(ds, N_IMAGES, N_RAND)
    tab = ds._device["tables"]
    R = len(picks) * per
    d = [torch.tensor(x, device=DEV) for x in (picks, pixels)] + [None if noise is None else torch.tensor(noise, device=DEV)]
    out = {k: torch.empty((R,) + ref.ROWS[k], dtype=torch.int64 if k in ("cam_idxs", "kp_idx") else torch.float32, device=DEV)
           for k in ref.KEYS}
    fn = _hip.lib().danbo_batch_gather
    args = [*(_hip.ptr(tab.get(k)) for k in ref.TABLES), len(ds), len(ds.bgs), ds.H, ds.W, *(_hip.ptr(x) for x in d), len(picks), per,
            int(ds.mask_image), *(_hip.ptr(out[k]) for k in ref.KEYS), _hip.stream()]
    times = []
    for block in range(6):
        for _ in range(warmup if block == 0 else 0):
            _hip.check(fn(*args), "danbo_batch_gather")
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            _hip.check(fn(*args), "danbo_batch_gather")
        e1.record()
        torch.cuda.synchronize()
        if block:
            times.append(e0.elapsed_time(e1) * 1e-3 / steps)
    moved = 2 * sum(v.numel() * v.element_size() for v in out.values()) + 4 * (len(picks) + R + (3 * R if noise is not None else 0))
    return (statistics.median(times), min(times), max(times)), moved


def loop_time(cfg, arr, images, tmp, name, extra, iters, warm):
    """run_nerf.train for `iters` iterations on the given images -> seconds per iteration between iteration `warm` and the last"""
    import torch
    import run_nerf
    from core import load_data as ld
    marks = {}

    def marked(it):
        for k, batch in enumerate(it):
            if k in (warm, iters - 1):
                torch.cuda.synchronize()
                marks[k] = time.perf_counter()
            yield batch

    def load_data(args, device=None, rank=0, world=1):
        it, render_data, attrs = ld.load_data(args, device=device, images=images, rank=rank, world=world)
        return marked(it), render_data, attrs

    n = len(images[0])
    argv = ["--config", cfg, "--basedir", tmp, "--expname", name, "--no_reload", "--syn_poses", str(n // 4), "--syn_cams", "4", "--syn_res",
            str(images[0].shape[1]), "--i_print", str(10 * iters), "--i_weights", str(10 * iters), "--i_testset", str(10 * iters),
            "--n_iters", str(iters)] + extra
    kept = run_nerf.load_data
    run_nerf.load_data = load_data
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            run_nerf.train(argv)
    finally:
        run_nerf.load_data = kept
    return (marks[iters - 1] - marks[warm]) / (iters - 1 - warm)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=300, help="iterations of each run_nerf.py run")
    ap.add_argument("--warm", type=int, default=50, help="iterations of each run before the clock starts")
    ap.add_argument("--runs", type=int, default=3, help="runs of either kind, alternating")
    ap.add_argument("--skip_loop", action="store_true")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("bench_batch.py measures on the GPU: none visible")
    assert a.images % 4 == 0 and a.images >= N_IMAGES
    print(f"{torch.cuda.get_device_name(0)}; torch CPU threads {torch.get_num_threads()}; {a.images} images of {a.res} x {a.res}, "
          f"batches of {N_IMAGES} images x {N_RAND // N_IMAGES} rays")
    arr, images = arrays(a.images, a.res)
    sync = torch.cuda.synchronize

    def to_device(batch):
        return {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in batch.items()}

    for label, flags in (("flags off", {}), ("--mask_image --perturb_bg", dict(mask_image=True, perturb_bg=True))):
        host, dev = dataset(arr, images, **flags), dataset(arr, images, **flags).to_device(DEV)
        nbytes = sum(t.numel() * t.element_size() for t in dev._device["tables"].values())
        print(f"[{label}] resident tables: {nbytes / 1e6:.1f} MB")
        t = blocks(lambda: to_device(host.sample_batch(N_IMAGES, N_RAND)), a.steps, a.warmup, sync)
        print(f"[{label}] (a) host path, sample_batch + one .to(device) per tensor: {ms(t)} per batch")
        t = blocks(lambda: host.sample_batch(N_IMAGES, N_RAND), a.steps, a.warmup, sync)
        print(f"[{label}] (a) of which sample_batch alone (numpy, no copy): {ms(t)} per batch")
        t = blocks(lambda: dev._draw(N_IMAGES, N_RAND, 0, 1), a.steps, a.warmup, sync)
        print(f"[{label}] (b) the draw alone (numpy generator; shared by both paths): {ms(t)} per batch")
        t = blocks(lambda: dev.sample_batch(N_IMAGES, N_RAND, on_device=True), a.steps, a.warmup, sync)
        print(f"[{label}] (b) device path, draw + staging copy + launch: {ms(t)} per batch")
        k, moved = kernel_time(dev, a.steps, a.warmup)
        print(f"[{label}] (b) danbo_batch_gather alone, device events around {a.steps} launches: {1e6 * k[0]:.1f} us per launch (five "
              f"blocks: {1e6 * k[1]:.1f} .. {1e6 * k[2]:.1f} us); {moved / 1e6:.2f} MB read + written = {moved / k[0] / 1e9:.0f} GB/s")
        del host, dev

    if a.skip_loop:
        return
    cfg = os.path.join(ROOT, "danbo-pytorch_amd", "configs", "perfcap", "danbo_fast.txt")
    times = {"host": [], "device": []}
    with tempfile.TemporaryDirectory() as tmp:
        for run in range(a.runs):
            for name, extra in (("host", []), ("device", ["--device_data"])):
                times[name].append(loop_time(cfg, arr, images, tmp, f"{name}{run}", extra, a.iters, a.warm))
    for name, t in times.items():
        print(f"(c) run_nerf.py, configs/perfcap/danbo_fast.txt, batches from the {name}: {1e3 * statistics.median(t):.3f} ms per "
              f"iteration (median of {a.runs} runs of {a.iters - 1 - a.warm} timed iterations, alternating; runs: "
              + ", ".join(f"{1e3 * x:.3f}" for x in t) + " ms)")


if __name__ == "__main__":
    main()
