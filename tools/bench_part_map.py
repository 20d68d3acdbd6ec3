"""Times the bone-assignment maps on the bench frame (bench.py's workload: 512 x 512 rays, 48 + 16 samples; dev tool).

    python tools/bench_part_map.py [--steps 40] [--warmup 5] > profiles/part_map_measured.txt

Printed, all on the same box in the same run:
  * the frame plain, with part_map='confd', with part_map='entropy' (each also with part_valid_only) and plain once more, every one
    through bench.py's own discipline (bench.timed: settle until two blocks agree, --warmup untimed frames, the median of five
    blocks that share --steps frames) -- ms per frame and the ratio to the plain frame of this run;
  * K2 (ops.gather_assign_blend16 on the coarse pass's compacted rows) without and with the 24 logits, and the two new kernels
    (ops.part_colors per pass and mode, ops.composite_colors for rgb0 and for rgb_map) on their own: HIP events around blocks of
    launches, two warm-up launches, five blocks of at least 0.2 s, the median block and the spread.
No target is set: the plain frame of the same run is the yardstick.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "danbo-pytorch_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

DEV = "cuda:0"


def timed_blocks(fn, min_block_s=0.2, blocks=5):
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
        out.append(1e3 * e0.elapsed_time(e1) / reps)
    return statistics.median(out), min(out), max(out), reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import torch
    import bench
    from core import hip_ops as ops
    if not torch.cuda.is_available():
        raise RuntimeError("bench_part_map.py measures on the GPU: none visible")
    eng, inp, _ = bench.build_workload(DEV, view=0)
    S, Sf = bench.N_SAMPLES, bench.N_IMPORTANCE
    frame_args = (inp["rays_o"], inp["rays_d"], inp["skts"], inp["bones"], inp["cyls"], inp["cam_idx"], S, Sf)
    R = len(inp["rays_o"])
    eng.refresh()
    print(f"bench frame: {R} rays x ({S} + {Sf}) samples, {torch.cuda.get_device_name(0)}; culled part maps exact: "
          f"{eng._part_exact_culled(ops.RELU)} (empty-space density <= 0)")

    # ---- the frame
    variants = [("plain", {}), ("confd", dict(part_map="confd")), ("entropy", dict(part_map="entropy")),
                ("confd, valid_only", dict(part_map="confd", part_valid_only=True)),
                ("entropy, valid_only", dict(part_map="entropy", part_valid_only=True)), ("plain again", {})]
    base = None
    for name, kw in variants:
        sec, _, info = bench.timed(lambda kw=kw: eng.render(*frame_args, chunk=4096, **kw), args.steps, args.warmup, None, DEV, False)
        base = sec if base is None else base
        print(f"frame {name}: {1e3 * sec:.3f} ms (median of {len(info['block_ms'])} blocks sharing {args.steps} frames, spread "
              f"{100 * info['spread']:.1f} %; {len(info['settle_ms'])} settle blocks) = {sec / base:.3f} x the plain frame; "
              f"{R * (S + Sf) / sec / 1e6:.1f} M ray-samples/s")

    # ---- the kernels on their own
    k = eng.render(*frame_args, chunk=4096, keep=True, part_map="confd")
    n0, n1 = int(k["count_coarse"]), int(k["count_fine"])
    print(f"rows inside a volume: coarse {n0} of {R * S}, importance {n1} of {R * Sf}; samples of weight > 0 in the final order: "
          f"{int((k['T_i'] > 0).sum())} of {R * (S + Sf)}")
    near, far = eng.near_far(inp["rays_o"], inp["rays_d"], inp["cyls"], inp["skts"])
    mask = ops.ray_bone_mask(inp["rays_o"], inp["rays_d"], inp["skts"], eng.align, eng.axis_scale, near, far)
    geo = ops.Geometry(inp["rays_o"], inp["rays_d"], inp["skts"], eng.align, eng.axis_scale, z=k["z_coarse"], ray_mask=mask)
    vols = eng.volumes(inp["bones"])
    bits, lst, cnt = ops.bone_cull(geo, compact=True)

    def report(name, fn):
        med, lo, hi, reps = timed_blocks(fn)
        print(f"{name}: {med:.1f} us (median of 5 blocks of {reps}; blocks {lo:.1f} .. {hi:.1f} us, spread {100 * (hi - lo) / med:.1f} %)")
        return med

    a = report("K2 coarse pass, no logits (gather_assign_blend16)", lambda: ops.gather_assign_blend16(geo, vols, bits, eng.aw, eng.assign16, lst, cnt, geo.M, False))
    b = report("K2 coarse pass, with the 24 logits             ", lambda: ops.gather_assign_blend16(geo, vols, bits, eng.aw, eng.assign16, lst, cnt, geo.M, True))
    print(f"K2 with logits / without: {b / a:.3f}")
    col = torch.empty(R, S, 3, device=DEV)
    col_f = torch.empty(R, Sf, 3, device=DEV)
    for mode in ("confd", "entropy"):
        for vo in (False, True):
            tag = f"{mode}{', valid_only' if vo else ''}"
            report(f"part_colors coarse rows ({tag})", lambda: ops.part_colors(k["confd_coarse"], mode, col, k["list_coarse"], k["count_coarse"],
                                                                                  bits=k["valid_bits"], valid_only=vo))
            report(f"part_colors importance rows ({tag})", lambda: ops.part_colors(k["confd_fine"], mode, col_f, k["list_fine"], k["count_fine"],
                                                                                      bits=k["valid_bits_fine"], valid_only=vo))
    out = torch.empty(R, 3, device=DEV)
    report("composite_colors rgb0 (identity order, all rays)", lambda: ops.composite_colors(col, k["weights_coarse"], bits_a=k["valid_bits"], out=out))
    report("composite_colors rgb_map (sorted order, all rays)", lambda: ops.composite_colors(col, k["T_i"], col_f, k["sorted_idxs"], k["valid_bits"],
                                                                                            k["valid_bits_fine"], out=out))


if __name__ == "__main__":
    main()
