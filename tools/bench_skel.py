"""Micro-benchmark of the skeleton overlay (csrc/k_skel.hip) on 16 frames of 1000 x 1000 and of 512 x 512, float32 and uint8 sources
(dev tool), with the settle / median-of-five convention of tools/micro_mesh.py (device events, warm-up, five blocks of at least
0.1 s each, the median block).  The scene is tests/skel_ref.py's: a jittered rest pose seen by ring cameras 3 units away.  Printed:
  * the streaming rates tools/probe/hbm_rate.py reports in the same run;
  * danbo_skel_project in microseconds;
  * danbo_skel_draw per size and source type: ms, the bytes it has to move (12 + 3 or 3 + 3 per pixel) over that time beside the
    copy rate, the pixels it painted, and whether the overlay has the bits of the serial restatement of csrc/skel_math.hpp.
The 16 float32 frames of 1000 x 1000 are 192 MB: they fit the 256 MiB last-level cache, which the repeated calls of a timing block
can profit from; the rate is reported for what it is, bytes needed over time.

    python tools/bench_skel.py > profiles/skel_measured.txt
"""
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

N_FRAMES = 16


def measure(size, copy_tbs):
    import skel_ref as ref
    from core import _hip
    from core.utils.skeleton_draw import bone_colours, skeleton3d_to_2d
    lib = _hip.lib()
    P = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    s = ref.scene(N_FRAMES, size, size, 7, focal_stride=2, with_centers=True)
    kps, w2c, focals, centers = (torch.tensor(a, device=DEV) for a in (s["kps"], ref.w2c_of(s["c2ws"]), s["focals"], s["centers"]))
    ends = torch.empty(N_FRAMES, 24, 4, dtype=torch.int32, device=DEV)

    def project():
        assert lib.danbo_skel_project(P(kps), P(w2c), P(focals), 2, P(centers), N_FRAMES, size, size, P(ends), st) == 0
    ms_p, reps_p = timed_ms(project)
    same_ends = ref.same_bits(ends.cpu().numpy(), ref.host_project(s["kps"], ref.w2c_of(s["c2ws"]), s["focals"], s["centers"], size, size))
    assert ref.same_bits(skeleton3d_to_2d(kps, s["c2ws"], size, size, s["focals"], s["centers"]).cpu().numpy(), ends.cpu().numpy())
    print(f"{size} x {size}: danbo_skel_project of {N_FRAMES} x 24 bones {1e3 * ms_p:.2f} us ({reps_p} per block; 1 launch; same bits as the "
          f"serial restatement: {same_ends})")
    rng = np.random.default_rng(size)
    frames = {"float32": torch.tensor(rng.random((N_FRAMES, size, size, 3), dtype=np.float32), device=DEV)}
    frames["uint8"] = (frames["float32"] * 255).to(torch.uint8)
    colours = torch.tensor(bone_colours(), device=DEV)
    out = torch.empty(N_FRAMES, size, size, 3, dtype=torch.uint8, device=DEV)
    pixels = N_FRAMES * size * size
    for kind, src in frames.items():
        for width in (3, 8):
            def draw():
                assert lib.danbo_skel_draw(P(src), int(kind == "float32"), P(ends), P(colours), width, N_FRAMES, size, size, P(out), st) == 0
            ms, reps = timed_ms(draw)
            n_bytes = pixels * ((12 if kind == "float32" else 3) + 3)
            t0 = time.perf_counter()
            want = ref.host_draw(src.cpu().numpy(), ends.cpu().numpy(), bone_colours(), width)
            t1 = time.perf_counter()
            got = out.cpu().numpy()
            painted = int((got != ref.quantise(src.cpu().numpy())).any(-1).sum())
            print(f"{size} x {size} {kind} width {width}: danbo_skel_draw of {N_FRAMES} frames {ms:.4f} ms ({reps} per block; 1 launch), "
                  f"{n_bytes / 1e6:.1f} MB needed -> {n_bytes / ms / 1e9:.2f} TB/s ({n_bytes / ms / 1e9 / copy_tbs:.2f} x the copy rate "
                  f"{copy_tbs:.2f} TB/s); at least {painted} of {pixels} pixels painted; serial restatement {1e3 * (t1 - t0):.0f} ms "
                  f"(same bits as the kernel: {ref.same_bits(got, want)})")


def main():
    probe = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "probe", "hbm_rate.py")], capture_output=True, text=True,
                           timeout=300, check=True).stdout
    print(probe.strip())
    copy_tbs = float(re.search(r"copy .*?([\d.]+) TB/s", probe).group(1))
    for size in (1000, 512):
        measure(size, copy_tbs)


if __name__ == "__main__":
    main()
