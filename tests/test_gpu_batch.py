"""GPU tests of the device-resident training batches (danbo_batch_gather, PoseImageDataset.to_device / sample_batch(on_device=True),
--device_data): the device path against the numpy host path and against the serial restatement of csrc/batch_math.hpp, bit for
bit; guard words; the staging hand-over; one fused training step from either batch; a short training run.  No test hands the kernel
an index out of range: the clamps are tests/test_batch_host.py's, on the restatement."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import batch_ref as ref
from helpers import DEV, ROOT, golden, hip_lib
from mesh_ref import GUARD, N_GUARD

pytestmark = pytest.mark.gpu
H, W = 16, 20
FLAGS = [dict(), dict(mask_image=True, perturb_bg=True)]


def assert_same_batch(dev, host, where=None):
    assert set(dev) == set(host) and dev["N_uniques"] == host["N_uniques"]
    for k in ref.KEYS:
        d, h = dev[k], host[k]
        assert d.is_cuda and d.is_contiguous() and d.dtype == h.dtype and d.shape == h.shape, (k, where)
        assert torch.equal(d.cpu(), h), (k, where)


def big_dataset(seed=0, n_codes=None, **flags):
    """32 images of 64 x 64 (core.load_data.synthetic_arrays) with random colours, fractional masks, two backgrounds and centres"""
    from core.load_data import PoseImageDataset, synthetic_arrays
    arr = synthetic_arrays(n_poses=8, n_cams=4, H=64, W=64, pose_seed=0)
    rng = np.random.default_rng(5)
    n = len(arr["c2ws"])
    imgs = rng.uniform(size=(n, 64, 64, 3)).astype(np.float32)
    fgs = rng.choice(np.array([0, 0.25, 1], np.float32), size=(n, 64, 64, 1))
    bgs = rng.uniform(size=(2, 64, 64, 3)).astype(np.float32)
    centers = (32 + rng.uniform(-2, 2, size=(n, 2))).astype(np.float32)
    cams = rng.permutation(n) if n_codes is None else np.arange(n) % n_codes
    return PoseImageDataset(imgs, fgs, bgs, rng.integers(0, 2, size=n), arr["c2ws"], arr["focals"], arr["kp3d"], arr["bones"], arr["skts"],
                            arr["rest_pose"], cam_idxs=cams, centers=centers, seed=seed, **flags)


# ----------------------------------------------------------------------------- device against host
@pytest.mark.parametrize("centers", [None, "f32"])
def test_device_batches_equal_the_host_batches(centers):
    for flags in FLAGS:
        for n_images, n_rand in ref.MATRIX:
            for rank, world in ((0, 1), (0, 2), (1, 2)):
                if n_images % world:
                    continue
                host, dev = ref.toy_dataset(centers, seed=3, **flags), ref.toy_dataset(centers, seed=3, **flags).to_device(DEV)
                for step in range(2):
                    assert_same_batch(dev.sample_batch(n_images, n_rand, rank, world, on_device=True),
                                      host.sample_batch(n_images, n_rand, rank, world), (flags, n_images, n_rand, rank, world, step))


@pytest.mark.parametrize("flags", FLAGS, ids=["plain", "mask_perturb"])
def test_device_batches_at_the_workloads_ray_count(flags):
    """16 images x 192 rays: several workgroups of either kind"""
    host, dev = big_dataset(**flags), big_dataset(**flags).to_device(DEV)
    for step in range(2):
        assert_same_batch(dev.sample_batch(16, 3072, on_device=True), host.sample_batch(16, 3072), step)
    assert_same_batch(dev.sample_batch(16, 3072, 1, 2, on_device=True), host.sample_batch(16, 3072, 1, 2), "rank 1 of 2")


# ----------------------------------------------------------------------------- the C entry against the restatement
def guarded_outputs(R, shift):
    """one device buffer per output with N_GUARD guard words on either side; shift: words by which the float payloads start off a
    16-byte boundary (0: the kernel moves pose rows as 16-byte tuples, otherwise word by word) -> ({key: whole buffer}, {key: view})"""
    bufs, views = {}, {}
    for k in ref.KEYS:
        idx = k in ("cam_idxs", "kp_idx")
        words = R * int(np.prod(ref.ROWS[k], dtype=np.int64)) * (2 if idx else 1)
        lead = N_GUARD + (0 if idx else shift)
        buf = torch.full((lead + words + N_GUARD,), GUARD, dtype=torch.int32, device=DEV)
        bufs[k] = (buf, lead, words)
        views[k] = buf[lead:lead + words].view(torch.int64 if idx else torch.float32).view((R,) + ref.ROWS[k])
    return bufs, views


def guards_intact(bufs):
    for k, (buf, lead, words) in bufs.items():
        b = buf.cpu().numpy().view(np.uint32)
        if not (np.all(b[:lead] == GUARD) and np.all(b[lead + words:] == GUARD)):
            return False
    return True


def call_entry(ds, per, picks, pixels, noise, shift=0):
    from core import _hip
    t = {k: (None if v is None else torch.tensor(v, device=DEV)) for k, v in ref.tables_of(ds).items()}
    R = len(picks) * per
    bufs, views = guarded_outputs(R, shift)
    d_picks, d_pixels = torch.tensor(picks, device=DEV), torch.tensor(pixels, device=DEV)
    d_noise = None if noise is None else torch.tensor(noise, device=DEV)
    assert d_picks.dtype == d_pixels.dtype == torch.int32
    rc = hip_lib().danbo_batch_gather(*(_hip.ptr(t[k]) for k in ref.TABLES), len(ds), len(ds.bgs), ds.H, ds.W, _hip.ptr(d_picks),
                                      _hip.ptr(d_pixels), _hip.ptr(d_noise), len(picks), per, int(ds.mask_image),
                                      *(_hip.ptr(views[k]) for k in ref.KEYS), _hip.stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    return bufs, {k: v.cpu().numpy() for k, v in views.items()}


@pytest.mark.parametrize("shift", [0, 1, 2], ids=["aligned", "off_by_4", "off_by_8"])
@pytest.mark.parametrize("centers", [None, "f32"])
def test_entry_equals_the_restatement_and_keeps_its_guards(centers, shift):
    assert hip_lib() is not None
    for flags in FLAGS:
        ds = ref.toy_dataset(centers, seed=7, **flags)
        per, picks, pixels, noise = ref.draw(ds, 4, 44)                      # 11 rays an image: the last pose group is short
        pixels[:4] = [0, H * W - 1, W - 1, (H - 1) * W]                      # the image's corners
        want = ref.host_gather(ref.tables_of(ds), H, W, per, picks, pixels, noise, ds.mask_image)
        bufs, got = call_entry(ds, per, picks, pixels, noise, shift)
        assert guards_intact(bufs)
        for k in ref.KEYS:
            assert ref.same_bits(got[k], want[k]), (k, flags)
        bufs2, again = call_entry(ds, per, picks, pixels, noise, shift)      # determinism: the same bits on a second call
        assert guards_intact(bufs2) and all(ref.same_bits(got[k], again[k]) for k in ref.KEYS)


def test_entry_at_the_workloads_ray_count_equals_the_restatement():
    ds = big_dataset(seed=2, mask_image=True, perturb_bg=True)
    per, picks, pixels, noise = ref.draw(ds, 16, 3072)
    pixels[:2] = [0, 64 * 64 - 1]
    want = ref.host_gather(ref.tables_of(ds), 64, 64, per, picks, pixels, noise, True)
    bufs, got = call_entry(ds, per, picks, pixels, noise)
    assert guards_intact(bufs) and all(ref.same_bits(got[k], want[k]) for k in ref.KEYS)


# ----------------------------------------------------------------------------- staging
def test_fifty_batches_without_a_synchronisation():
    """the two pinned staging buffers are rewritten only after the copy that read them: no batch sees a later batch's draws"""
    flags = dict(mask_image=True, perturb_bg=True)
    host, dev = ref.toy_dataset("f32", seed=11, **flags), ref.toy_dataset("f32", seed=11, **flags).to_device(DEV)
    got = [dev.sample_batch(4, 64, on_device=True) for _ in range(50)]
    torch.cuda.synchronize()
    for step, b in enumerate(got):
        assert_same_batch(b, host.sample_batch(4, 64), step)


def test_device_batches_drawn_from_sampling_masks():
    masks = np.zeros((6, H, W), np.uint8)
    masks[:, 3:9, 5:12] = 1
    masks[1] = 0                                         # an empty mask: that image's pixels come from the whole image
    flags = dict(sampling_masks=masks, mask_image=True, perturb_bg=True)
    host, dev = ref.toy_dataset("f32", seed=5, **flags), ref.toy_dataset("f32", seed=5, **flags).to_device(DEV)
    for step in range(4):
        assert_same_batch(dev.sample_batch(4, 64, on_device=True), host.sample_batch(4, 64), step)


def test_to_device_refuses_tables_the_entry_cannot_take():
    from core.load_data import PoseImageDataset
    kw = ref.toy_arrays()
    with pytest.raises(ValueError, match=r"c2ws must be \[6, 4, 4\]"):          # (3 x 4 cameras serve the host path under masks)
        PoseImageDataset(**dict(kw, c2ws=kw["c2ws"][:, :3]), sampling_masks=np.ones((6, H, W))).to_device(DEV)
    with pytest.raises(ValueError, match="bg_idxs outside"):
        ds = ref.toy_dataset()
        ds.bg_idxs = ds.bg_idxs + 1
        ds.to_device(DEV)


def test_tables_that_do_not_fit_raise_with_the_byte_counts(monkeypatch):
    ds = ref.toy_dataset()
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda device=None: (1000, 2000))
    with pytest.raises(RuntimeError, match=r"take \d+ bytes, 1000 of 2000 bytes are free"):
        ds.to_device(DEV)
    assert ds._device is None


# ----------------------------------------------------------------------------- training
def test_one_fused_step_from_either_batch_gives_the_same_bits():
    """The step's inputs are equal bit for bit, and so is every output the engine computes without atomics: the maps, alphas,
    weights and counters.  Its four loss terms and the flat gradient are float-atomic sums, whose bits depend on the order of
    arrival even when one engine repeats one batch (test_gpu_train_engine.py::test_graph_replays_are_repeatable, which bounds that
    at 1e-5 of the largest entry); they are held to that bound here.  Measured on an MI355X between the two batches: loss terms
    0, 3.1e-7, 5.3e-7 and 0 relative, the gradient 7.5e-9 of a largest entry of 2.9e-2 (2.6e-7)."""
    from test_gpu_training import build_trainer
    g = golden("danbo_perfcap_train")
    S, Sf = int(g["N_samples"]), int(g["N_importance"])
    flags = dict(mask_image=True, perturb_bg=True, n_codes=int(g["n_framecodes"]))
    batches = [big_dataset(**flags).sample_batch(16, 3072), big_dataset(**flags).to_device(DEV).sample_batch(16, 3072, on_device=True)]
    results = []
    for b in batches:
        args, caster, trainer, opt = build_trainer(g)
        eng = trainer.fused_engine()
        assert eng is not None, trainer.fused_reason
        eng.use_graph = False
        b = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in b.items()}
        G, pp = b["N_uniques"], caster._per_pose
        out = eng.forward_backward(b["rays_o"], b["rays_d"], pp(b["skts"], G), pp(b["bones"], G), pp(b["cyls"], G), b["cam_idxs"],
                                   b["target_s"], b["bgs"], S, Sf)
        torch.cuda.synchronize()
        results.append(({k: v.clone() for k, v in out.items() if torch.is_tensor(v)}, eng.flat_g.clone()))
    for k in ref.KEYS:
        assert torch.equal(batches[0][k].to(DEV), batches[1][k]), k
    (out_h, g_h), (out_d, g_d) = results
    exact = {"rgb_map", "disp_map", "acc_map", "alpha", "weights", "rgb0", "disp0", "acc0", "alpha0", "counts"}
    assert set(out_h) == set(out_d) == exact | {"loss"}
    for k in sorted(exact):
        assert torch.equal(out_h[k], out_d[k]), k
    rel = ((out_h["loss"] - out_d["loss"]).abs() / out_h["loss"].abs()).tolist()       # each term against itself: their sizes differ
    print("loss terms", out_h["loss"].tolist(), "relative differences", rel)
    assert bool(torch.isfinite(out_h["loss"]).all()) and max(rel) <= 1e-5
    d, top = float((g_h - g_d).abs().max()), float(g_h.abs().max())
    print(f"gradient: max difference {d:.3e} of {top:.3e}")
    assert bool(torch.isfinite(g_h).all()) and top > 0 and d <= 1e-5 * top
    assert float(out_h["acc_map"].max()) > 0            # the rays met the volumes: the step did its work


def test_short_training_run_on_device_data(tmp_path):
    cfg = os.path.join(ROOT, "danbo-pytorch_amd", "configs", "surreal", "danbo_fast.txt")
    cmd = [sys.executable, os.path.join(ROOT, "danbo-pytorch_amd", "run_nerf.py"), "--config", cfg, "--basedir", str(tmp_path), "--expname",
           "dev", "--syn_poses", "2", "--syn_cams", "2", "--syn_res", "32", "--syn_rest_scale", "0.714", "--N_rand", "512",
           "--N_sample_images", "4", "--i_print", "5", "--i_weights", "20", "--i_testset", "1000", "--n_iters", "20", "--device_data",
           "--mask_image", "--perturb_bg"]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-3000:]
    log = tmp_path / "dev"
    assert (log / "000020.tar").exists()
    text = (log / "args.txt").read_text()
    assert "device_data = True" in text and "mask_image = True" in text and "perturb_bg = True" in text
    losses = [json.loads(line)["Stats/total_loss"] for line in open(log / "scalars.jsonl")]
    assert len(losses) == 4 and np.isfinite(losses).all()
