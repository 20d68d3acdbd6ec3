"""A/B of the density activation on the bench frame (dev tool): the config-1 frame through DanboEngine.render with relu, with relu
and the rays-of-constants shortcut off, and with softplus (which has no such rays), interleaved; then the composites alone.
    python tools/ab_density_act.py [--shift 1.0]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "danbo-pytorch_amd"))
import numpy as np
import torch
import bench
from core import hip_ops as ops

ap = argparse.ArgumentParser()
ap.add_argument("--shift", type=float, default=1.0)
a = ap.parse_args()
SP = ("softplus", a.shift)
eng, inp, _ = bench.build_workload(torch.device("cuda:0"), 0)
args = (inp["rays_o"], inp["rays_d"], inp["skts"], inp["bones"], inp["cyls"], inp["cam_idx"], 48, 16)


def frame(act, skip_flat):
    eng.cfg["density_act"], eng.skip_flat_rays = act, skip_flat
    try:
        return eng.render(*args)
    finally:
        eng.cfg["density_act"], eng.skip_flat_rays = ops.RELU, True


cases = {"relu": (ops.RELU, True), "relu, no rays of constants": (ops.RELU, False), "softplus": (SP, True)}
for _ in range(30):
    for c in cases.values():
        frame(*c)
torch.cuda.synchronize()
res = {k: [] for k in cases}
for rep in range(8):
    for name, c in cases.items():
        for _ in range(5):
            frame(*c)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(20):
            frame(*c)
        torch.cuda.synchronize(); res[name].append((time.perf_counter() - t0) / 20 * 1e3)
for k, v in res.items():
    print("frame, %-28s ms median %.4f  min %.4f max %.4f" % (k, float(np.median(v)), min(v), max(v)))
out = frame(SP, True)
print("softplus frame: acc_map min %.4f, share of rays with acc = 1: %.3f" % (float(out["acc_map"].min()), float((out["acc_map"] >= 1).float().mean())))

# ---- the composites alone, on the relu frame's tensors
k = eng.render(*args, keep=True)
_, raw_empty = eng.view_constants(inp["rays_d"], inp["skts"], inp["cam_idx"])
z, raw, bits, d = k["z_coarse"], k["raw_coarse"], k["valid_bits"], inp["rays_d"]
bits_f, _, _ = ops.bone_cull(ops.Geometry(inp["rays_o"], d, inp["skts"], eng.align, eng.axis_scale, z=k["z_fine"]), True)


def timeit(fn, reps=20):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps


for name, act in (("relu", ops.RELU), ("softplus", SP)):
    print("composite_importance, all rays, %-9s us %.1f" % (name, timeit(lambda: ops.composite_importance(
        raw, z, d, 16, 1.0, bits=bits, raw_empty=raw_empty, want_weights=False, act=act))))
    print("composite_merged,     all rays, %-9s us %.1f" % (name, timeit(lambda: ops.composite_merged(
        raw, k["raw_fine"], k["sorted_idxs"], k["z_sorted"], d, 1.0, bits_a=bits, bits_b=bits_f, raw_empty=raw_empty, act=act))))
    print("composite (unfused),  all rays, %-9s us %.1f" % (name, timeit(lambda: ops.composite(
        raw, z, d, 1.0, bits=bits, raw_empty=raw_empty, act=act))))
