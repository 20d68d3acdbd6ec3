"""First measurement of the depth and normal maps (csrc/k_depth.hip) at the bench frame's shape -- 512 x 512 rays, 48 + 16 samples
(dev tool).  One run, device events, every shape warmed up, a settle block, then blocks of at least 0.2 s each; the median block
with the lowest and the highest beside it.  Printed:
  * the streaming rates tools/probe/hbm_rate.py reports in the same run (the box's copy rate);
  * danbo_depth_composite_fwd alone on the bench frame's own final weights and sorted depths (keep=True render): all rays, and the
    listed rays only (the list of the rays that are not rays of constants, as render(depth=True) calls it); microseconds, the
    bytes the launch needs (8 n per ray read, 8 per ray written) over that time beside the copy rate; same bits as the serial
    restatement of csrc/depth_math.hpp on a sample of the rays;
  * danbo_depth_normals alone on the assembled 512 x 512 frame: the bytes it needs (depth, acc and the cast mask read once, 12
    written per pixel);
  * the bench frame (bench.py's render) with and without depth=True, the two alternating block by block in this same run: the
    figure to read is the difference of the medians, with the spread of either beside it.

    python tools/bench_depth.py > profiles/depth_measured.txt
"""
import ctypes
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "danbo-pytorch_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402

DEV = "cuda:0"
BLOCKS, MIN_BLOCK_S = 7, 0.2


def block_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def timed(fns):
    """every function of `fns` warmed up and settled, then BLOCKS blocks each, alternating between the functions block by block
    -> [(median ms, lowest, highest, calls per block)] in the order of fns"""
    reps = []
    for fn in fns:
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        reps.append(max(1, int(MIN_BLOCK_S * 1e3 / max(block_ms(fn, 1), 1e-3)) + 1))
    for fn, r in zip(fns, reps):
        block_ms(fn, r)                      # settle: clocks and caches as the timed blocks find them
    out = [[] for _ in fns]
    for _ in range(BLOCKS):
        for i, (fn, r) in enumerate(zip(fns, reps)):
            out[i].append(block_ms(fn, r))
    return [(statistics.median(o), min(o), max(o), r) for o, r in zip(out, reps)]


def show(ms):
    return f"{ms[0] * 1e3:.1f} us (blocks {ms[1] * 1e3:.1f} .. {ms[2] * 1e3:.1f} us, {ms[3]} calls each)"


def rate(n_bytes, ms, copy_tbs):
    tbs = n_bytes / (ms[0] * 1e-3) / 1e12
    return f"{n_bytes / 1e6:.1f} MB needed -> {tbs:.2f} TB/s ({tbs / copy_tbs:.2f} x the copy rate {copy_tbs:.2f} TB/s)"


def main():
    import bench
    import depth_ref as ref
    from core import _hip, hip_ops as ops
    probe = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "probe", "hbm_rate.py")], capture_output=True, text=True,
                           timeout=300, check=True).stdout
    print(probe.strip())
    copy_tbs = float(re.search(r"copy .*?([\d.]+) TB/s", probe).group(1))
    S, Sf, H, W = bench.N_SAMPLES, bench.N_IMPORTANCE, bench.H, bench.W
    n = S + Sf
    eng, inp, _ = bench.build_workload(DEV, 0)
    args = (inp["rays_o"], inp["rays_d"], inp["skts"], inp["bones"], inp["cyls"], inp["cam_idx"], S, Sf)
    keep = eng.render(*args, keep=True)
    w, z = keep["T_i"].contiguous(), keep["z_sorted"].contiguous()
    R = w.shape[0]
    near, far = eng.near_far(inp["rays_o"], inp["rays_d"], inp["cyls"], inp["skts"])
    mask = ops.ray_bone_mask(inp["rays_o"], inp["rays_d"], inp["skts"], eng.align, eng.axis_scale, near, far, want_flat=True)
    flat = ops.flat_rays(mask[1], mask[3], S, Sf)
    listed = int(flat["ray_count"])
    print(f"bench frame: {H} x {W} = {R} rays, {S} + {Sf} samples; {listed} rays listed ({R - listed} rays of constants); "
          f"rays with acc >= 0.5: {int((keep['acc_map'] >= 0.5).sum())}")

    # ---- the two launches alone
    lib = _hip.lib()
    P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())      # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = torch.zeros(2, R, device=DEV)

    def composite_all():
        assert lib.danbo_depth_composite_fwd(P(w), P(z), R, n, 0.5, None, None, P(out[0]), P(out[1]), st) == 0

    def composite_listed():
        assert lib.danbo_depth_composite_fwd(P(w), P(z), R, n, 0.5, P(flat["ray_list"]), P(flat["ray_count"]), P(out[0]), P(out[1]), st) == 0
    ms_all, ms_listed = timed([composite_all, composite_listed])
    composite_all()
    torch.cuda.synchronize()
    pick = np.random.default_rng(0).choice(R, 4096, replace=False)
    want = ref.host_composite(w.cpu().numpy()[pick], z.cpu().numpy()[pick], 0.5)
    same = ref.same_bits(out[0].cpu().numpy()[pick], want[0]) and ref.same_bits(out[1].cpu().numpy()[pick], want[1])
    print(f"danbo_depth_composite_fwd, all {R} rays, n = {n}: {show(ms_all)}; 1 launch; {rate(R * (8 * n + 8), ms_all, copy_tbs)}; "
          f"same bits as the serial restatement on 4096 rays: {same}")
    print(f"danbo_depth_composite_fwd, the {listed} listed rays: {show(ms_listed)}; 1 launch; "
          f"{rate(listed * (8 * n + 8 + 4), ms_listed, copy_tbs)}")

    depth = out[0].reshape(1, H, W).contiguous()
    acc = keep["acc_map"].reshape(1, H, W).contiguous()
    cast = torch.ones(1, H, W, dtype=torch.uint8, device=DEV)
    c2w = torch.eye(4, device=DEV)[None, :3].contiguous()
    intr = torch.tensor([[500.0, 500.0, W / 2, H / 2]], device=DEV)
    rgb = torch.empty(1, H, W, 3, device=DEV)
    valid = torch.empty(1, H, W, dtype=torch.uint8, device=DEV)

    def normals():
        assert lib.danbo_depth_normals(P(depth), P(acc), P(cast), P(c2w), P(intr), 1, H, W, 0.5, 0.0, 0, 1.0, P(rgb), P(valid), st) == 0
    ms_n, = timed([normals])
    torch.cuda.synchronize()
    want = ref.host_normals(depth.cpu().numpy(), acc.cpu().numpy(), cast.cpu().numpy(), c2w.cpu().numpy(), intr.cpu().numpy())
    same = ref.same_bits(rgb.cpu().numpy(), want[0]) and ref.same_bits(valid.cpu().numpy(), want[1])
    print(f"danbo_depth_normals, 1 frame of {H} x {W}: {show(ms_n)}; 1 launch; {rate(H * W * (4 + 4 + 1 + 12 + 1), ms_n, copy_tbs)}; "
          f"{int(valid.sum())} pixels with a normal; same bits as the serial restatement: {same}")

    # ---- the bench frame with and without depth=True, alternating
    plain = lambda: eng.render(*args, chunk=4096)                    # noqa: E731
    deep = lambda: eng.render(*args, chunk=4096, depth=True)          # noqa: E731
    a, b = plain(), deep()
    same = all(torch.equal(a[k], b[k]) for k in a)
    ms_plain, ms_deep = timed([plain, deep])
    fmt = lambda m: f"{m[0]:.4f} ms (blocks {m[1]:.4f} .. {m[2]:.4f} ms, {m[3]} frames each)"      # noqa: E731
    print(f"bench frame, plain render: {fmt(ms_plain)}")
    print(f"bench frame, depth=True:   {fmt(ms_deep)}; every other map bit for bit the plain render's: {same}")
    extra = ms_deep[0] - ms_plain[0]
    print(f"extra time of depth=True over the plain frame of the same run: {extra * 1e3:.1f} us ({100 * extra / ms_plain[0]:.2f} % of the frame; "
          f"spread of the plain blocks {1e3 * (ms_plain[2] - ms_plain[1]):.1f} us, of the depth blocks {1e3 * (ms_deep[2] - ms_deep[1]):.1f} us)")


if __name__ == "__main__":
    main()
