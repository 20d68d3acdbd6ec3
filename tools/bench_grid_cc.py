"""Micro-benchmark of the grid components and the floater filter (csrc/k_grid_cc.hip) on 256^3 grids (dev tool), with the settle /
median-of-five convention of tools/micro_mesh.py (device events, warm-up, five blocks of at least 0.1 s each, the median block).
Three grids: the golden pose's density grid of tools/micro_mesh.py (the x-y swapped view RayCaster.render_mesh_density returns,
threshold = the median of its positive values, floor 0), its analytic sphere, and a p = 0.5 Bernoulli grid (the many-components
worst case).  Printed per grid:
  * danbo_grid_cc_label, danbo_grid_cc_keep (keep_largest) and their sum in ms, the statistics, and whether labels, sizes, stats and
    the filtered grid have the bits of the serial restatement of csrc/grid_cc_math.hpp;
  * the label call against its traffic floor: 4 B read + 8 B written per point at the read rate tools/probe/hbm_rate.py reports;
and what they are to be judged against, from the same run:
  1. the host path they replace: device -> host copy, scipy.ndimage.label, bincount, mask, host -> device copy;
  2. danbo_mesh_count + danbo_mesh_extract on the same grid;
  3. render_mesh_density at the same resolution (golden pose only), which precedes them.

    python tools/bench_grid_cc.py [--res 255] > profiles/grid_cc_measured.txt
"""
import argparse
import ctypes
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "danbo-pytorch_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from micro_mesh import DEV, timed_ms  # noqa: E402


def host_path(sigma, iso, floor):
    """copy to the host, label, bincount, mask, copy back -> (ms of each step, the filtered grid on the device)"""
    from scipy import ndimage
    torch.cuda.synchronize()
    t = [time.perf_counter()]
    host = sigma.contiguous().cpu().numpy()
    t.append(time.perf_counter())
    inside = np.maximum(np.nan_to_num(host, nan=-np.inf), np.float32(floor)) >= np.float32(iso)
    lab, n = ndimage.label(inside)
    t.append(time.perf_counter())
    if n:
        counts = np.bincount(lab.reshape(-1))
        counts[0] = 0
        host = np.where(inside & (lab != counts.argmax()), np.float32(floor if floor < iso else -np.inf), host)
    t.append(time.perf_counter())
    back = torch.tensor(host, device=DEV)
    torch.cuda.synchronize()
    t.append(time.perf_counter())
    return [1e3 * (b - a) for a, b in zip(t, t[1:])], back, n


def measure(name, sigma, iso, floor, read_tbs):
    from core import _hip
    import grid_cc_ref as ref
    lib = _hip.lib()
    nx, ny, nz = sigma.shape
    n = nx * ny * nz
    P = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    grid = (P(sigma), nx, ny, nz, sigma.stride(0), sigma.stride(1), floor, iso)
    ws = torch.empty(lib.danbo_grid_cc_workspace_bytes(nx, ny, nz), dtype=torch.uint8, device=DEV)
    labels, sizes = (torch.empty(n, dtype=torch.int32, device=DEV) for _ in range(2))
    stats, kept = torch.empty(4, dtype=torch.int32, device=DEV), torch.empty(2, dtype=torch.int32, device=DEV)
    out = torch.empty_strided(sigma.shape, sigma.stride(), dtype=torch.float32, device=DEV)
    fill = floor if floor < iso else float("-inf")

    def label():
        assert lib.danbo_grid_cc_label(*grid, P(ws), P(labels), P(sizes), P(stats), st) == 0

    def keep():
        assert lib.danbo_grid_cc_keep(*grid, P(labels), P(sizes), P(stats), 1, 0, fill, P(out), out.stride(0), out.stride(1), P(kept), st) == 0
    ms_l, reps_l = timed_ms(label)
    ms_k, reps_k = timed_ms(keep)
    floor_ms = 12 * n / (read_tbs * 1e9)
    print(f"{name}: grid {nx} x {ny} x {nz} ({4 * n / 1e6:.1f} MB, strides {tuple(sigma.stride())}), iso {iso:.6g}, floor {floor}; stats "
          f"(inside, components, largest, its label) {stats.tolist()}, kept (components, points) {kept.tolist()}")
    print(f"{name}: danbo_grid_cc_label {ms_l:.4f} ms ({reps_l} per block; 5 launches), traffic floor (4 B read + 8 B written per point) "
          f"{floor_ms:.4f} ms at {read_tbs:.2f} TB/s -> {ms_l / floor_ms:.1f} x the floor")
    print(f"{name}: danbo_grid_cc_keep (keep_largest) {ms_k:.4f} ms ({reps_k} per block; 2 launches); label + keep {ms_l + ms_k:.4f} ms")
    # the bits, against the serial restatement
    host = np.ascontiguousarray(sigma.cpu().numpy())
    t0 = time.perf_counter()
    want = ref.host_label(host, iso, floor)
    want_out, want_kept = ref.host_keep(host, iso, floor, *want, keep_largest=True, fill=fill)
    t1 = time.perf_counter()
    same = (all(ref.same_bits(a.cpu().numpy().reshape(b.shape), b) for a, b in zip((labels, sizes, stats), want))
            and ref.same_bits(out.cpu().numpy(), want_out) and ref.same_bits(kept.cpu().numpy(), want_kept))
    print(f"{name}: serial restatement {1e3 * (t1 - t0):.1f} ms (same bits as the kernels: {same})")
    # 1. the host path
    steps, back, n_comp = host_path(sigma, iso, floor)
    steps, back, n_comp = host_path(sigma, iso, floor)        # (the second run: pages and pools are warm)
    agree = bool(((back.clamp(min=floor) >= iso) == (out.clamp(min=floor) >= iso)).all())
    print(f"{name}: host path: device -> host {steps[0]:.1f} ms + scipy.ndimage.label {steps[1]:.1f} ms + bincount and mask {steps[2]:.1f} ms "
          f"+ host -> device {steps[3]:.1f} ms = {sum(steps):.1f} ms ({n_comp} components; the same inside set: {agree}) -> "
          f"{sum(steps) / (ms_l + ms_k):.0f} x label + keep")
    # 2. the extraction on the same grid
    mws = torch.empty(lib.danbo_mesh_workspace_bytes(nx, ny, nz), dtype=torch.uint8, device=DEV)
    counts = torch.zeros(2, dtype=torch.int32, device=DEV)

    def count():
        assert lib.danbo_mesh_count(*grid, P(mws), P(counts), st) == 0
    count()
    V, T = counts.tolist()
    verts = torch.empty(max(V, 1), 3, dtype=torch.float32, device=DEV)
    tris = torch.empty(max(T, 1), 3, dtype=torch.int32, device=DEV)

    def extract():
        assert lib.danbo_mesh_extract(*grid, P(mws), 1.0, 0., 0., 0., P(verts), V, P(tris), T, st) == 0
    ms_c, _ = timed_ms(count)
    ms_e, _ = timed_ms(extract)
    print(f"{name}: danbo_mesh_count + danbo_mesh_extract {ms_c:.4f} + {ms_e:.4f} = {ms_c + ms_e:.4f} ms (V {V}, T {T}) -> label + keep = "
          f"{(ms_l + ms_k) / (ms_c + ms_e):.1f} x the extraction")
    return ms_l + ms_k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=255)
    args = ap.parse_args()
    probe = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "probe", "hbm_rate.py")], capture_output=True, text=True,
                           timeout=300, check=True).stdout
    print(probe.strip())
    read_tbs = float(re.search(r"sum .*?([\d.]+) TB/s", probe).group(1))
    from helpers import golden
    from test_gpu_modules import build, T
    import mesh_ref
    g = golden("danbo_mesh")
    caster, _ = build("h36m_zju/danbo_base.txt", g)
    pose = (T(g["kps"][:1]), T(g["skts"][:1]), T(g["bones"][:1]))
    kw = dict(fwd_type="mesh", radius=float(g["radius"]), res=args.res)
    with torch.no_grad():
        dens = caster(*pose, **kw)
        ms_d, reps_d = timed_ms(lambda: caster(*pose, **kw), min_block_s=0.0)
    print(f"render_mesh_density res {args.res}: {ms_d:.2f} ms ({reps_d} per block)")
    pos = dens[dens > 0]
    iso = float(pos.median()) if pos.numel() else 0.0
    ms = measure("golden pose", dens, iso, 0.0, read_tbs)
    print(f"golden pose: (label + keep) / render_mesh_density = {ms / ms_d:.5f}")
    n = args.res + 1
    sphere = torch.tensor(mesh_ref.sphere_grid((n, n, n), R=0.39 * n, centre=(0.497 * n, 0.502 * n, 0.493 * n)), device=DEV)
    measure("sphere", sphere, 0.0, float("-inf"), read_tbs)
    noise = torch.tensor(np.where(np.random.default_rng(0).random((n, n, n)) < 0.5, np.float32(1), np.float32(-1)), device=DEV)
    measure("bernoulli p = 0.5", noise, 0.0, float("-inf"), read_tbs)


if __name__ == "__main__":
    main()
