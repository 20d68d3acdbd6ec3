"""The set-up of a motion of 4096 frames in front of the renderer, timed three ways (dev tool; first measurements, no target):
  * the existing host path: run_render._pose_chain (get_smpl_l2ws pose by pose, np.linalg.inv) on all 4096 poses, and
    get_kp_bounding_cylinder + kp_to_valid_rays (the rays of the whole image made on the device, copied to the host, indexed by
    the box there) on the first HOST_FRAMES frames, scaled to 4096 -- at 1000 x 1000 the whole motion would take minutes and hold
    tens of GB of rays on the host;
  * the device path: core.motion.pose_chain on all 4096 poses and core.motion.frame_rays on all 4096 frames, in chunks of CHUNK
    frames whose rays are dropped before the next (all boxes of 1000 x 1000 frames at once are tens of GB on the device too);
  * the three launches alone: danbo_pose_rotations and danbo_pose_chain on 4096 poses, danbo_box_rays on the motion's median box,
    with the settle / median-of-five convention of tools/micro_mesh.py (device events, warm-up, five blocks of at least 0.1 s).
The path timings are host clocks around work that ends in a device synchronise, the median of three runs after one warm-up run.
The motion: 4096 seeded poses with joint angles up to 0.6 rad at the origin, seen by one camera 3 units away, focal 1.25 x the
image size (the synthetic data's).  Checked in the same run: the device's boxes and ray counts are the host path's on the frames
both made.

    python tools/bench_motion.py > profiles/motion_measured.txt
"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "danbo-pytorch_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from micro_mesh import DEV, timed_ms  # noqa: E402

FRAMES, HOST_FRAMES, CHUNK, EXT_SCALE = 4096, 128, 512, 0.00035


def clocked(fn, runs=3):
    """-> (median, min, max) seconds of `runs` runs of fn after one warm-up run, each ended by a device synchronise"""
    out = []
    for i in range(runs + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    out = out[1:]
    return statistics.median(out), min(out), max(out)


def line(name, t, scale=1.0):
    med, lo, hi = (1e3 * scale * x for x in t)
    return f"{name}: {med:.1f} ms (runs {lo:.1f} .. {hi:.1f} ms)"


def main():
    import motion_ref as mr
    import run_render
    import core.motion as cm
    from core import _hip
    from core.load_data import generate_bullet_time
    from core.utils.ray_utils import kp_to_valid_rays
    print(f"{torch.cuda.get_device_name(0)}; torch {torch.__version__}; first measurements, no target")
    print(f"motion: {FRAMES} seeded poses, joint angles <= 0.6 rad, one camera 3 units away, focal 1.25 x the image size")
    bones, rest = mr.random_bones(FRAMES, seed=0, max_angle=0.6), mr.rest_pose()
    roots = np.zeros((FRAMES, 3), np.float32)
    base = np.eye(4, dtype=np.float32)
    base[2, 3] = 3.0
    c2ws = np.repeat(generate_bullet_time(base, 4)[1:2].astype(np.float32), FRAMES, 0)
    d_bones, d_rest, d_roots = (torch.tensor(a, device=DEV) for a in (bones, rest, roots))

    # ---- the chain
    host = {}

    def host_chain():
        host["kps"], host["skts"] = run_render._pose_chain(bones, rest.astype(np.float64), roots[:, None])
    t_host_chain = clocked(host_chain, runs=1)
    chain = {}

    def dev_chain():
        chain.update(cm.pose_chain(bones=d_bones, rest_pose=d_rest, roots=d_roots, ext_scale=EXT_SCALE))
    t_dev_chain = clocked(dev_chain)
    err = np.abs(chain["kps"].cpu().numpy() - host["kps"]).max()
    print(line(f"host chain, {FRAMES} poses (_pose_chain: get_smpl_l2ws pose by pose + np.linalg.inv; 1 run after the warm-up)", t_host_chain))
    print(line(f"device chain, {FRAMES} poses (core.motion.pose_chain: 2 launches, 4 output tensors allocated)", t_dev_chain)
          + f"; largest joint difference to the host chain {err:.2e}")

    # ---- the three launches alone
    P, st = _hip.ptr, _hip.stream()
    lib = cm.lib()
    rots = torch.empty(FRAMES, 24, 3, 3, device=DEV)

    def k_rot():
        assert lib.danbo_pose_rotations(P(d_bones), FRAMES, P(rots), st) == 0

    def k_chain():
        assert lib.danbo_pose_chain(P(rots), P(d_rest), P(d_roots), FRAMES, P(chain["l2ws"]), P(chain["skts"]), P(chain["kps"]),
                                    P(chain["cyls"]), *cm.cylinder_extensions(EXT_SCALE), st) == 0
    for name, fn, n_bytes in (("danbo_pose_rotations", k_rot, FRAMES * 24 * (12 + 36)),
                              ("danbo_pose_chain", k_chain, FRAMES * (24 * (36 + 64 + 64 + 12) + 12 + 20))):
        ms, reps = timed_ms(fn)
        print(f"{name}, {FRAMES} poses: {1e3 * ms:.1f} us ({reps} calls per block; 1 launch; {n_bytes / 1e6:.2f} MB read and written)")

    # ---- the rays
    for size in (512, 1000):
        focal = np.full(FRAMES, 1.25 * size, np.float32)
        d_poses = torch.tensor(c2ws, device=DEV)
        made = {}

        def host_rays():
            made["host"] = kp_to_valid_rays(d_poses[:HOST_FRAMES], size, size, focal[:HOST_FRAMES], kps=chain["kps"][:HOST_FRAMES],
                                            ext_scale=EXT_SCALE)

        def dev_rays():
            counts, boxes = [], []
            for s in range(0, FRAMES, CHUNK):
                e = s + CHUNK
                rays, idxs, _, bx = cm.frame_rays(c2ws[s:e], size, size, focal[s:e], chain["kps"][s:e], chain["cyls"][s:e])
                counts += [len(i) for i in idxs]
                boxes += bx
            made["dev"] = (counts, boxes)
        t_host = clocked(host_rays)
        t_dev = clocked(dev_rays)
        counts, boxes = made["dev"]
        h_rays, h_idxs, _, h_boxes = made["host"]
        same = all(np.array_equal(boxes[i][0], h_boxes[i][0]) and np.array_equal(boxes[i][1], h_boxes[i][1]) and counts[i] == len(h_idxs[i])
                   for i in range(HOST_FRAMES))
        med = int(np.argsort(counts)[len(counts) // 2])
        tl, br = boxes[med]
        print(f"---- {size} x {size}: boxes of {min(counts)} .. {max(counts)} rays, median {counts[med]} ({br[0] - tl[0]} x {br[1] - tl[1]}); "
              f"boxes and ray counts of the first {HOST_FRAMES} frames equal to the host path's: {same}")
        print(line(f"host rays, {HOST_FRAMES} frames (get_kp_bounding_cylinder + kp_to_valid_rays)", t_host)
              + f" = {1e3 * t_host[0] / HOST_FRAMES:.2f} ms per frame, {t_host[0] / HOST_FRAMES * FRAMES:.1f} s for {FRAMES} frames at that rate")
        print(line(f"device rays, {FRAMES} frames (core.motion.frame_rays in chunks of {CHUNK}: {FRAMES // CHUNK} reads of cylinders, "
                   f"{FRAMES} launches, boxes on the host)", t_dev) + f" = {1e3 * t_dev[0] / FRAMES:.3f} ms per frame")
        host_all = t_host_chain[0] + t_host[0] / HOST_FRAMES * FRAMES
        dev_all = t_dev_chain[0] + t_dev[0]
        print(f"set-up of the {FRAMES}-frame motion at {size} x {size}: host path {host_all:.1f} s (chain measured, rays scaled from "
              f"{HOST_FRAMES} frames), device path {dev_all:.2f} s: {host_all / dev_all:.0f} x")
        n = counts[med]
        o, d, idx = torch.empty(n, 3, device=DEV), torch.empty(n, 3, device=DEV), torch.empty(n, dtype=torch.int64, device=DEV)

        def k_rays():
            assert lib.danbo_box_rays(P(d_poses[med]), float(focal[med]), float(focal[med]), size * 0.5, size * 0.5, size, int(tl[0]),
                                      int(tl[1]), int(br[0]), int(br[1]), P(o), P(d), P(idx), st) == 0
        ms, reps = timed_ms(k_rays)
        print(f"danbo_box_rays, the median box ({n} rays): {1e3 * ms:.1f} us ({reps} calls per block; 1 launch; {n * 32 / 1e6:.2f} MB written)")


if __name__ == "__main__":
    main()
