"""The oracle ON THE BENCH FRAME: centre rays of the 512 x 512 frame bench.py times, for BASELINE configs 1, 2
and 3 -- the HIP path's coarse-pass logits against oracle/torch_cpu.py (float32, and the same restatement in float64) TWICE: at the
HIP path's own depths and with the oracle's near / far fed in; the bounds themselves; the in-volume mask.  The dictionary asserted
here is the `parity` object of the bench line (bench.parity_block), so the line and the suite cannot disagree.

Why two comparisons: one ulp of a bound moves every sample of the ray, and this network turns a 5e-7 shift of the depths into 5e-4
of a logit (tools/diag/config2_bounds_attribution.py: the ORACLE'S OWN logits move by 4.6e-4 when it samples at bounds that differ
from its own by <= 1.7e-6) -- round 4's config-2 figure of 4.8e-4 was exactly that.  Since round 5 the box bounds follow the
reference's arithmetic to the bit (torch.norm's fma chain, the float32 1.3 bound: tests/test_host_logic.py), so both comparisons
must hold."""
import os
import sys

import numpy as np
import pytest
import torch

from helpers import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_RAYS = 4096


@pytest.mark.parametrize("config", [1, 2, 3])
def test_oracle_on_the_bench_frame(config):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import bench
    import torch_cpu
    from core.utils import synthetic as syn
    S, Sf, box = bench.CONFIGS[config]
    bench.N_SAMPLES, bench.N_IMPORTANCE = S, Sf
    eng, inp, extra = bench.build_workload(torch.device(DEV), view=0)
    eng.cfg["use_volume_near_far"] = box
    cfg, sd, rest, scene, ro, rd = extra
    out = eng.render(inp["rays_o"], inp["rays_d"], inp["skts"], inp["bones"], inp["cyls"], inp["cam_idx"], S, Sf, chunk=4096, keep=True)
    H = W = 512
    r0 = (H // 2) * W - N_RAYS // 2
    r0 -= r0 % 4096                                   # the sample's 4096-ray chunks are chunks of the frame (the cylinder's nan-mean)
    sl = slice(r0, r0 + N_RAYS)
    model = torch_cpu.DanboTorchCPU(dict(cfg, use_volume_near_far=box), sd, rest)
    z = np.zeros(N_RAYS, dtype=np.int64)
    ref = model.render(syn.ray_batch(ro[sl], rd[sl]), scene["skts"][z], scene["bones"][z], scene["cyls"][z], np.zeros(N_RAYS, np.int64), 1,
                       S, Sf, stages=True)
    stages = dict(raw_coarse=out["raw_coarse"], valid_bits=out["valid_bits"], near=out["near"], far=out["far"], Sf=Sf)
    p = bench.parity_block(model, extra, sl, ref, out, stages, eng_inp=(eng, inp))
    print({k: v for k, v in p.items() if k != "raw_note"})
    # bounds: the box bounds are the reference's to the bit; the cylinder's differ where torch's CPU pow(x, 0.5) is not sqrt (not at
    # all on the oracle side) and in the summation order of the chunk's nan-mean
    assert p["max_abs_near"] <= bench.BOUNDS_BOUND and p["max_abs_far"] <= bench.BOUNDS_BOUND
    if box:
        assert p["bounds_bit_equal_rays"] == N_RAYS, "box bounds must equal the oracle's bit for bit"
    for side in ("own_depths", "oracle_depths"):
        q = p[side]
        assert q["mask_mismatches"] == 0, side
        if side == "own_depths" and p["bounds_bit_equal_rays"] != N_RAYS:
            continue        # not the same function of the same depths: reported, decided at the oracle's depths
        assert q["max_rel_raw_floored_5pct"] <= 1e-4, (side, q)
        assert q["max_rel_raw_floored_5pct_vs_float64"] <= 1e-4, (side, q)
        assert q["max_rel_raw"] <= 1e-4 and q["max_rel_raw_vs_float64"] <= 1e-4, (side, q)
    assert p["parity_ok"] is True and p["parity_ok_timed_frame"] is True
    # the maps of the timed frame against the oracle's, after importance resampling
    assert p["max_abs_rgb"] < 1e-4 and p["max_abs_acc"] < 1e-4 and p["psnr_rgb_db"] > 90.0


def test_plain_bench_run_dumps_the_outputs_of_its_last_timed_frame(tmp_path):
    """`bench.py --steps K --warmup W --dump-outputs DIR` without --full: EXACTLY K timed steps, the headline fields and none of
    what --full adds; DIR holds the outputs of the last timed frame (float32, <= 64 MB, a fixed sample of the rows of the large
    ones), bit for bit those of the same frame rendered here."""
    import json
    import subprocess
    sys.path.insert(0, ROOT)
    import bench
    got_dir, ref_dir = tmp_path / "bench", tmp_path / "here"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--dump-outputs", str(got_dir)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    r = json.loads(lines[0])
    assert r["steps"] == 3 and sum(r["block_steps"]) == 3 and r["ms_per_step"] > 0 and r["higher_is_better"] is True
    assert r["unit"] == "ray-samples/s" and abs(r["value"] - 512 * 512 * 64 / (r["ms_per_step"] * 1e-3)) <= 1e-9 * r["value"]
    assert not {"roofline", "sparsity", "cpu_baseline", "parity", "api_value", "dense_value", "occupancy_sweep"} & set(r)
    got = {f.stem: np.load(f) for f in got_dir.glob("*.npy")}
    assert sum(a.nbytes for a in got.values()) <= 64 << 20 and all(a.dtype == np.float32 for a in got.values())
    assert got["rgb_map"].shape == (512 * 512, 3) and 0 < got["alpha"].shape[0] < 512 * 512 and got["alpha"].shape[1] == 64
    bench.N_SAMPLES, bench.N_IMPORTANCE, box = bench.CONFIGS[1]
    eng, inp, _ = bench.build_workload(torch.device(DEV), view=0)
    eng.cfg["use_volume_near_far"] = box
    out = bench.render(eng, inp)
    bench.dump_outputs(str(ref_dir), {k: v for k, v in out.items() if torch.is_tensor(v)})
    assert sorted(got) == sorted(f.stem for f in ref_dir.glob("*.npy"))
    for k, a in got.items():
        np.testing.assert_array_equal(a, np.load(ref_dir / f"{k}.npy"), err_msg=k)
