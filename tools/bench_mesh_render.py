"""Times the 91-frame turntable of a res-255 mesh at 512 x 512 (csrc/k_raster.hip through core/utils/mesh_render.render_turntable;
dev tool).  The mesh is the isosurface of a synthetic density grid -- a torus or a sphere, extracted by the library's own marching
cubes with vertex normals -- so no checkpoint is needed.

    python tools/bench_mesh_render.py [--shape torus] [--res 255] [--size 512 512] [--out DIR] > profiles/mesh_render_measured.txt

Printed:
  * the turntable (91 frames, uint8 stack on the device): ms per turntable and per frame -- device events around whole turntables,
    two warm-up turntables, five blocks of at least 0.5 s each, the median block and the spread (min .. max of the blocks);
  * the rasteriser alone (hip_ops.rasterize_mesh of the 91 views into float images, no uint8 conversion) the same way;
  * with --out DIR: the split over the four stages (k_raster_vertices / clear / depth / resolve) from ONE
    `rocprofv3 --kernel-trace --stats` run of a fresh child process (this file with --child: three turntables), taken before this
    process touches the GPU; the kernel_stats csv stays in DIR.
There is no earlier implementation to compare with (the reference draws with OpenGL): these are first measurements, no threshold.
"""
import argparse
import csv
import glob
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "danbo-pytorch_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

DEV = "cuda:0"
STAGES = ("k_raster_vertices", "k_raster_clear", "k_raster_depth", "k_raster_resolve")


def density_grid(shape, res):
    """a signed distance (positive inside) on the (res + 1)^3 grid, made on the device"""
    import torch
    n = res + 1
    t = torch.arange(n, dtype=torch.float32, device=DEV)
    x, y, z = torch.meshgrid(t - 0.497 * n, t - 0.502 * n, t - 0.493 * n, indexing="ij")
    if shape == "sphere":
        return 0.39 * n - torch.sqrt(x * x + y * y + z * z)
    return 0.12 * n - torch.sqrt((torch.sqrt(x * x + y * y) - 0.3 * n) ** 2 + z * z)


def make_mesh(shape, res):
    from core import hip_ops
    return hip_ops.marching_cubes(density_grid(shape, res), 0.0, scale=1.0 / res, offset=(-.5, -.5, -.5), normals=True)


def timed_blocks(fn, min_block_s=0.5, blocks=5):
    import torch
    fn()
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    reps = max(1, int(min_block_s * 1e3 / max(e0.elapsed_time(e1), 1e-3)) + 1)
    out = []
    for _ in range(blocks):
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / reps)
    return statistics.median(out), min(out), max(out), reps


def stage_split(out_dir, args):
    """one rocprofv3 --kernel-trace --stats run of a child process -> {stage: (calls, total ns)}"""
    os.makedirs(out_dir, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out_dir, "-o", "mesh_render", "--",
           sys.executable, os.path.abspath(__file__), "--child", "--shape", args.shape, "--res", str(args.res), "--size", *map(str, args.size)]
    subprocess.run(cmd, check=True, timeout=600, stdout=subprocess.DEVNULL)
    files = sorted(glob.glob(os.path.join(out_dir, "**", "*kernel_stats.csv"), recursive=True))
    if not files:
        raise RuntimeError(f"rocprofv3 left no kernel_stats.csv under {out_dir}")
    split = {}
    with open(files[-1]) as f:
        for row in csv.DictReader(f):
            for s in STAGES:
                if s in row["Name"]:
                    calls, ns = split.get(s, (0, 0))
                    split[s] = (calls + int(row["Calls"]), ns + int(row["TotalDurationNs"]))
    return split, files[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="torus", choices=["torus", "sphere"])
    ap.add_argument("--res", type=int, default=255)
    ap.add_argument("--size", type=int, nargs=2, default=[512, 512])
    ap.add_argument("--out", default=None, help="directory for the rocprofv3 run (the stage split); without it the split is skipped")
    ap.add_argument("--child", action="store_true", help="three turntables and nothing else (what rocprofv3 traces)")
    args = ap.parse_args()
    split = None
    if args.out and not args.child:
        split = stage_split(args.out, args)           # a fresh child under the profiler, before this process opens the GPU
    import torch
    from core import hip_ops
    from core.utils import mesh_render as mr
    if not torch.cuda.is_available():
        raise RuntimeError("bench_mesh_render.py measures on the GPU: none visible")
    H, W = args.size
    verts, faces, normals = make_mesh(args.shape, args.res)
    turntable = lambda: mr.render_turntable(verts, faces, normals=normals, size=(H, W))      # noqa: E731
    if args.child:
        for _ in range(3):
            turntable()
        torch.cuda.synchronize()
        return
    views = mr.turntable_views(verts)
    raster = lambda: [hip_ops.rasterize_mesh(verts, faces, normals, views=views[j:j + 16], half_extent=mr.HALF_EXTENT, size=(H, W))      # noqa: E731
                      for j in range(0, len(views), 16)]
    frames = turntable()
    covered = float((frames != 255).any(-1).float().mean())
    print(f"mesh: {args.shape}, res {args.res}: V {len(verts)}, T {len(faces)}; {len(views)} frames of {H} x {W}, "
          f"{100 * covered:.1f} % of the pixels covered; {torch.cuda.get_device_name(0)}")
    for name, fn in (("turntable (views + rasteriser + uint8 frames)", turntable), ("rasteriser alone (float images)", raster)):
        med, lo, hi, reps = timed_blocks(fn)
        print(f"{name}: {med:.3f} ms per turntable, {med / len(views):.4f} ms per frame (median of 5 blocks of {reps}; "
              f"blocks {lo:.3f} .. {hi:.3f} ms, spread {100 * (hi - lo) / med:.1f} %)")
    if split is not None:
        stats, path = split
        total = sum(ns for _, ns in stats.values())
        print(f"stages (rocprofv3 --kernel-trace --stats, 3 turntables = {3 * len(views)} frames, {os.path.relpath(path, args.out)}):")
        for s in STAGES:
            calls, ns = stats.get(s, (0, 0))
            print(f"  {s}: {calls} launches, {ns / max(calls, 1) / 1e3:.2f} us per launch, {100 * ns / max(total, 1):.1f} % of the four")
        print(f"  the four stages: {total / (3 * len(views)) / 1e6:.4f} ms of kernel time per frame")


if __name__ == "__main__":
    main()
