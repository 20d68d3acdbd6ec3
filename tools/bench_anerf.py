"""A-NeRF frame timing for SURVEY §8(d) config 5: anerf_base network, 512 x 512 rays x (48 + 16) samples,
tau = 20 (step 0) or 2000 (converged).  Every sample is evaluated (A-NeRF has no in-volume mask).
--two-net: the anerf_h sampling with a separate fine network (single_net = False): 96 + 48 samples, the coarse network on the 96,
the fine network on all 144 -- 240 network rows per ray (AnerfEngine.render_two_net).
    python tools/bench_anerf.py [--steps 3] [--warmup 1] [--tau 20] [--hw 512] [--two-net]
Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "danbo-pytorch_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--tau", type=float, default=20.0)
    ap.add_argument("--hw", type=int, default=512)
    ap.add_argument("--rows-per-chunk", type=int, default=1 << 20)
    ap.add_argument("--two-net", action="store_true")
    a = ap.parse_args()
    from core.anerf_engine import AnerfEngine
    from core.utils import synthetic as syn
    from core.utils.skeleton_utils import bone_align_transforms
    dev = torch.device("cuda:0")
    cfg = syn.model_config("anerf_base")
    rest = syn.rest_pose(cfg["rest_scale"])
    sd = syn.make_state_dict(cfg, seed=0, n_framecodes=100, rest=rest)
    sd["pe_fn.tau"] = np.array(a.tau, np.float32)
    sd["dirs_pe_fn.tau"] = np.array(a.tau, np.float32)
    scene = syn.make_scene(n_poses=1, H=a.hw, W=a.hw, n_views=8, pose_seed=0, min_radius=1.25)
    ro, rd = scene["rays"][0]
    T = lambda x, dt=torch.float32: torch.tensor(np.ascontiguousarray(x), dtype=dt, device=dev)  # noqa: E731
    eng = AnerfEngine(cfg, {k: T(v) for k, v in sd.items()}, T(bone_align_transforms(rest)), rows_per_chunk=a.rows_per_chunk)
    inp = dict(rays_o=T(ro), rays_d=T(rd), skts=T(scene["skts"]), bones=T(scene["bones"]), cyls=T(scene["cyls"]),
               cam_idx=torch.zeros(len(ro), dtype=torch.int64, device=dev))
    S, Sf = (96, 48) if a.two_net else (48, 16)
    if a.two_net:
        sd_f = syn.make_state_dict(cfg, seed=1, n_framecodes=100, rest=rest)
        sd_f["pe_fn.tau"], sd_f["dirs_pe_fn.tau"] = sd["pe_fn.tau"], sd["dirs_pe_fn.tau"]
        fine = AnerfEngine(cfg, {k: T(v) for k, v in sd_f.items()}, T(bone_align_transforms(rest)), rows_per_chunk=a.rows_per_chunk)
        run = lambda: eng.render_two_net(fine, inp["rays_o"], inp["rays_d"], inp["skts"], inp["bones"], inp["cyls"],  # noqa: E731
                                         inp["cam_idx"], S, Sf)
    else:
        run = lambda: eng.render(inp["rays_o"], inp["rays_d"], inp["skts"], inp["bones"], inp["cyls"], inp["cam_idx"], S, Sf)  # noqa: E731
    for _ in range(a.warmup):
        out = run()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(a.steps + 1)]
    ev[0].record()
    for i in range(a.steps):
        out = run()
        ev[i + 1].record()
    torch.cuda.synchronize()
    each = [ev[i].elapsed_time(ev[i + 1]) for i in range(a.steps)]
    ms = sum(each) / a.steps
    # network rows per ray: S + Sf for one network (the importance samples only go through it a second time), S + (S + Sf) for two
    n = len(ro) * ((2 * S + Sf) if a.two_net else (S + Sf))
    W, inc, VW = cfg["W"], 432, cfg["view_W"]
    mac = inc * W + 4 * W * W + (inc + W) * W + 2 * W * W + W + W * VW + 24 * VW + 3 * VW
    print(json.dumps(dict(metric="ray-samples/s", value=n / ms * 1e3, ms_per_frame=ms, ms_each=each, rays=len(ro),
                          samples_per_ray=S + Sf, two_net=a.two_net, network_rows_per_ray=n // len(ro),
                          tau=a.tau, executed_mac_per_sample=mac, reference_mac_per_sample=2268000,
                          tflops_executed=n * mac * 2 / ms / 1e9, acc_mean=float(out["acc_map"].mean()),
                          config=("anerf_base network, anerf_h sampling (96 + 48), two networks" if a.two_net else
                                  "h36m_zju/anerf_base (SURVEY 8d config 5)") + ", k_linear16 trunk (fp16-split MFMA)")))


if __name__ == "__main__":
    main()
