"""Micro-benchmark of the isosurface extraction (csrc/k_mesh.hip) on 256^3 grids (dev tool): the golden pose's density grid (the
x-y swapped view RayCaster.render_mesh_density returns, threshold = the median of its positive values, floor 0) and an analytic
sphere.  Device events, warm-up, five blocks of at least 0.1 s each, the median block.  Printed per grid:
  * danbo_mesh_count (classify + scan) and danbo_mesh_extract (vertices + triangles) in ms, V and T;
  * the classify pass against its read floor: the grid's bytes / the read rate tools/probe/hbm_rate.py reports in the same run;
  * render_mesh_density of the same grid (the step the extraction follows);
  * the host path it replaces: device -> host copy of the grid + the serial extractor of csrc/mesh_math.hpp.

    python tools/micro_mesh.py [--res 255] > profiles/mesh_extract_measured.txt

--normals: instead, on the same two grids, danbo_mesh_normals (k_mesh_normals) beside k_mesh_vertices alone (danbo_mesh_extract with
a triangle capacity of 0) from the same run, and the normals against the serial restatement of csrc/mesh_math.hpp.

    python tools/micro_mesh.py --normals > profiles/mesh_attrs_measured.txt
"""
import argparse
import ctypes
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "danbo-pytorch_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402

DEV = "cuda:0"


def timed_ms(fn, min_block_s=0.1, blocks=5):
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
    return statistics.median(out), reps


def measure(name, sigma, iso, floor, read_tbs):
    from core import _hip
    import mesh_ref
    lib = _hip.lib()
    nx, ny, nz = sigma.shape
    P = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ws = torch.empty(lib.danbo_mesh_workspace_bytes(nx, ny, nz), dtype=torch.uint8, device=DEV)
    counts = torch.zeros(2, dtype=torch.int32, device=DEV)
    grid = (P(sigma), nx, ny, nz, sigma.stride(0), sigma.stride(1), floor, iso)

    def count():
        assert lib.danbo_mesh_count(*grid, P(ws), P(counts), st) == 0
    count()
    V, T = counts.tolist()
    verts = torch.empty(max(V, 1), 3, dtype=torch.float32, device=DEV)
    tris = torch.empty(max(T, 1), 3, dtype=torch.int32, device=DEV)

    def extract():
        assert lib.danbo_mesh_extract(*grid, P(ws), 1.0, 0., 0., 0., P(verts), V, P(tris), T, st) == 0
    ms_c, reps_c = timed_ms(count)
    ms_e, reps_e = timed_ms(extract)
    n_bytes = 4 * nx * ny * nz
    floor_ms = n_bytes / (read_tbs * 1e9)
    inside = int((torch.clamp(sigma, min=floor) >= iso).sum())
    print(f"{name}: grid {nx} x {ny} x {nz} ({n_bytes / 1e6:.1f} MB, strides {tuple(sigma.stride())}), iso {iso:.6g}, floor {floor}, "
          f"inside {inside}, V {V}, T {T}")
    print(f"{name}: danbo_mesh_count (classify + scan) {ms_c:.4f} ms ({reps_c} launches per block), read floor {floor_ms:.4f} ms at "
          f"{read_tbs:.2f} TB/s -> {ms_c / floor_ms:.2f} x the floor; workspace {ws.numel() / 1e6:.1f} MB")
    print(f"{name}: danbo_mesh_extract (vertices + triangles) {ms_e:.4f} ms ({reps_e} launches per block); count + extract "
          f"{ms_c + ms_e:.4f} ms")
    # the host path: copy of the grid + the serial extractor
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host = sigma.contiguous().cpu().numpy()
    t1 = time.perf_counter()
    hv, hf = mesh_ref.host_extract(host, iso, floor, check_guards=False)
    t2 = time.perf_counter()
    same = hv.tobytes() == verts[:V].cpu().numpy().tobytes() and hf.tobytes() == tris[:T].cpu().numpy().tobytes()
    print(f"{name}: host path: device -> host copy {1e3 * (t1 - t0):.1f} ms + serial extractor {1e3 * (t2 - t1):.1f} ms "
          f"(same bits as the kernels: {same})")
    return ms_c + ms_e


def measure_normals(name, sigma, iso, floor):
    from core import _hip
    import mesh_attr_ref
    lib = _hip.lib()
    nx, ny, nz = sigma.shape
    P = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ws = torch.empty(lib.danbo_mesh_workspace_bytes(nx, ny, nz), dtype=torch.uint8, device=DEV)
    counts = torch.zeros(2, dtype=torch.int32, device=DEV)
    grid = (P(sigma), nx, ny, nz, sigma.stride(0), sigma.stride(1), floor, iso)
    assert lib.danbo_mesh_count(*grid, P(ws), P(counts), st) == 0
    V, T = counts.tolist()
    verts = torch.empty(max(V, 1), 3, dtype=torch.float32, device=DEV)
    normals = torch.empty(max(V, 1), 3, dtype=torch.float32, device=DEV)

    def vertices():
        assert lib.danbo_mesh_extract(*grid, P(ws), 1.0, 0., 0., 0., P(verts), V, None, 0, st) == 0

    def nrm():
        assert lib.danbo_mesh_normals(*grid, P(ws), P(normals), V, st) == 0
    ms_v, reps_v = timed_ms(vertices)
    ms_n, reps_n = timed_ms(nrm)
    print(f"{name}: grid {nx} x {ny} x {nz} (strides {tuple(sigma.stride())}), iso {iso:.6g}, floor {floor}, V {V}, T {T}")
    print(f"{name}: k_mesh_vertices {ms_v:.4f} ms ({reps_v} launches per block); k_mesh_normals (danbo_mesh_normals) {ms_n:.4f} ms "
          f"({reps_n} launches per block) = {ms_n / ms_v:.2f} x")
    t0 = time.perf_counter()
    want = mesh_attr_ref.host_normals(sigma.contiguous().cpu().numpy(), iso, floor)
    t1 = time.perf_counter()
    same = want.tobytes() == normals[:V].cpu().numpy().tobytes()
    print(f"{name}: serial restatement {1e3 * (t1 - t0):.1f} ms (same bits as the kernel: {same})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=255)
    ap.add_argument("--normals", action="store_true", help="time danbo_mesh_normals beside k_mesh_vertices instead")
    args = ap.parse_args()
    if args.normals:
        return main_normals(args)
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
    print(f"golden pose: extraction / render_mesh_density = {ms / ms_d:.5f}")
    n = args.res + 1
    sphere = torch.tensor(mesh_ref.sphere_grid((n, n, n), R=0.39 * n, centre=(0.497 * n, 0.502 * n, 0.493 * n)), device=DEV)
    measure("sphere", sphere, 0.0, float("-inf"), read_tbs)


def main_normals(args):
    from helpers import golden
    from test_gpu_modules import build, T
    import mesh_ref
    g = golden("danbo_mesh")
    caster, _ = build("h36m_zju/danbo_base.txt", g)
    with torch.no_grad():
        dens = caster(T(g["kps"][:1]), T(g["skts"][:1]), T(g["bones"][:1]), fwd_type="mesh", radius=float(g["radius"]), res=args.res)
    pos = dens[dens > 0]
    measure_normals("golden pose", dens, float(pos.median()) if pos.numel() else 0.0, 0.0)
    n = args.res + 1
    sphere = torch.tensor(mesh_ref.sphere_grid((n, n, n), R=0.39 * n, centre=(0.497 * n, 0.502 * n, 0.493 * n)), device=DEV)
    measure_normals("sphere", sphere, 0.0, float("-inf"))


if __name__ == "__main__":
    main()
