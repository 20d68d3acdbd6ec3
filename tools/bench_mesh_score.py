"""First measurement of the mesh scores (csrc/k_mesh_score.hip) at 10^5 x 10^5 and 2.7 x 10^5 x 2.7 x 10^5 points -- 2.7 x 10^5 is the
vertex count of the res-255 mesh (dev tool).  One run, device events, every shape warmed up, a settle block, then blocks of at least
0.2 s each; the median block with the lowest and the highest beside it.  Printed per size:
  * the four launches alone: danbo_mesh_face_areas and danbo_mesh_sample on an icosphere of 81 920 faces, danbo_points_nearest in
    both directions between the samples of two such spheres (radii 1 and 1.1), danbo_points_score with normals and two thresholds;
    for the sweep also the pairs per second and the VALU instructions per pair and lane-cycle that rate amounts to on 256 CUs x 64
    lanes at 2.4 GHz (arithmetic, not a target);
  * score_points end to end (both directions, both reductions, the one host read);
  * beside it, when scipy imports, scipy.spatial.cKDTree on the host on the same points: the copies of the two point sets to the
    host, building both trees, querying both directions (one thread and 16 threads);
  * whether d2 and idx of a sample of the queries have the bits of the serial restatement of csrc/mesh_score_math.hpp.

    python tools/bench_mesh_score.py > profiles/mesh_score_measured.txt
"""
import datetime
import os
import socket
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "danbo-pytorch_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402

DEV = "cuda:0"
BLOCKS, MIN_BLOCK_S = 5, 0.2
SIZES = (100_000, 270_000)
TAUS = (0.01, 0.02)
CHECKED = 256                   # queries compared with the restatement
HOST_THREADS = 16               # of the cKDTree queries' second timing


def block_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def timed(fn):
    """fn warmed up and settled, then BLOCKS blocks -> (median ms, lowest, highest, calls per block)"""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    reps = max(1, int(MIN_BLOCK_S * 1e3 / max(block_ms(fn, 1), 1e-3)) + 1)
    block_ms(fn, reps)
    o = [block_ms(fn, reps) for _ in range(BLOCKS)]
    return statistics.median(o), min(o), max(o), reps


def show(ms):
    unit, k = ("us", 1e3) if ms[0] < 1 else ("ms", 1.0)
    return f"{ms[0] * k:.1f} {unit} (blocks {ms[1] * k:.1f} .. {ms[2] * k:.1f} {unit}, {ms[3]} calls each)"


def main():
    import mesh_score_ref as ref
    from core import mesh_score as ms
    print(f"{socket.gethostname()}, {torch.cuda.get_device_name(0)}, {datetime.date.today().isoformat()}; "
          f"torch {torch.__version__}; first measurements, no target")
    T = lambda x, dt=torch.float32: torch.tensor(np.ascontiguousarray(x), dtype=dt, device=DEV)      # noqa: E731
    va, fa = ref.icosphere(6, 1.0)
    vb, fb = ref.icosphere(6, 1.1)
    print(f"meshes: two icospheres of {len(va)} vertices and {len(fa)} faces, radii 1 and 1.1")
    va_t, fa_t, vb_t, fb_t = T(va), T(fa, torch.int32), T(vb), T(fb, torch.int32)
    try:
        from scipy.spatial import cKDTree
    except Exception as e:      # noqa: BLE001
        cKDTree = None
        print(f"scipy.spatial.cKDTree: not measured (scipy does not import: {type(e).__name__})")
    for n in SIZES:
        print(f"---- {n} x {n} points")
        gen = torch.Generator(device=DEV)
        gen.manual_seed(0)
        cdf_a, u_a = ms.sample_inputs(va_t, fa_t, n, gen)
        gen.manual_seed(1)
        cdf_b, u_b = ms.sample_inputs(vb_t, fb_t, n, gen)
        print(f"danbo_mesh_face_areas, {len(fa)} faces: {show(timed(lambda: ms.face_areas(va_t, fa_t)))} (with the wrapper's flag read)")
        print(f"danbo_mesh_sample, {n} samples: {show(timed(lambda: ms.sample_with(va_t, fa_t, cdf_a, u_a)))} (with the wrapper's flag read)")
        pa, na, _ = ms.sample_with(va_t, fa_t, cdf_a, u_a)
        pb, nb, _ = ms.sample_with(vb_t, fb_t, cdf_b, u_b)
        splits = ref.host_lib().ref_splits(n, n)
        for name, q, r in (("a -> b", pa, pb), ("b -> a", pb, pa)):
            t = timed(lambda: ms.nearest(q, r))
            pairs = float(n) * n / (t[0] * 1e-3)
            print(f"danbo_points_nearest {name}: {show(t)}; {splits} reference splits; {pairs / 1e12:.2f} x 10^12 pairs/s = "
                  f"{256 * 64 * 2.4e9 / pairs:.1f} lane-cycles per pair on 256 CUs x 64 lanes at 2.4 GHz")
        d2, idx = ms.nearest(pa, pb)
        print(f"danbo_points_score, {n} queries, normals, {len(TAUS)} thresholds: {show(timed(lambda: ms.direction_sums(d2, idx, na, nb, TAUS)))}")
        t = timed(lambda: ms.score_points(pa, na, pb, nb, TAUS))
        s = ms.score_points(pa, na, pb, nb, TAUS)
        print(f"score_points end to end (two sweeps, two reductions, one host read): {show(t)}")
        print(f"  chamfer_l1 {s['chamfer_l1']:.6f} chamfer_l2 {s['chamfer_l2']:.6f} normal_consistency {s['normal_consistency']:.6f} "
              f"fscore {s['fscore']}")
        # the restatement's bits on a sample of the queries (the whole reference set)
        pick = np.linspace(0, n - 1, CHECKED).astype(np.int64)
        pa_h, pb_h = pa.cpu().numpy(), pb.cpu().numpy()
        hd2, hidx = ref.host_nearest(pa_h[pick], pb_h)
        same = ref.same_bits(d2.cpu().numpy()[pick], hd2) and ref.same_bits(idx.cpu().numpy()[pick], hidx)
        print(f"same bits as the serial restatement on {CHECKED} queries (d2 and idx): {same}")
        if cKDTree is not None:
            t0 = time.perf_counter()
            pa_h, pb_h = pa.cpu().numpy(), pb.cpu().numpy()
            t1 = time.perf_counter()
            ta, tb = cKDTree(pa_h), cKDTree(pb_h)
            t2 = time.perf_counter()
            da, ia = tb.query(pa_h)
            db, _ = ta.query(pb_h)
            t3 = time.perf_counter()
            tb.query(pa_h, workers=HOST_THREADS)
            ta.query(pb_h, workers=HOST_THREADS)
            t4 = time.perf_counter()
            agree = float(np.mean(ia == idx.cpu().numpy()))
            print(f"scipy.spatial.cKDTree on the host, both directions: copies to the host {1e3 * (t1 - t0):.1f} ms, two trees "
                  f"{1e3 * (t2 - t1):.1f} ms, queries {1e3 * (t3 - t2):.1f} ms on one thread ({1e3 * (t4 - t3):.1f} ms on "
                  f"{HOST_THREADS} threads): {1e3 * (t3 - t0):.1f} ms in all; chamfer_l1 {0.5 * (da.mean() + db.mean()):.6f}; the "
                  f"same index as the sweep on {100 * agree:.2f} % of the queries (float64 distances break near-ties differently)")


if __name__ == "__main__":
    main()
