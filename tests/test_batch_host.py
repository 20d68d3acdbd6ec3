"""Training batches (mask_image / perturb_bg / sampling_masks, danbo_batch_gather), the part that needs no GPU: the host path's
batch semantics, the serial restatement of csrc/batch_math.hpp against the numpy host path bit for bit, its clamps, the binding of
include/danbo_batch.h, the argument checks (which return before any launch) and the new flags."""
import ctypes
import os

import numpy as np
import pytest
import torch

import batch_ref as ref
from helpers import ADDR as P, EINVAL, ROOT, entry        # P: an address no check follows

H, W = 16, 20
FLAGS = [dict(), dict(mask_image=True), dict(perturb_bg=True), dict(mask_image=True, perturb_bg=True)]


def batches_equal(a, b):
    assert set(a) == set(b) == set(ref.KEYS) | {"N_uniques"} and a["N_uniques"] == b["N_uniques"]
    return all(ref.same_bits(a[k].numpy(), b[k].numpy()) for k in ref.KEYS)


# ----------------------------------------------------------------------------- the host path
def parent_sample_batch(ds, N_images, N_rand, rank=0, world=1):
    """sample_batch as it was before the flags existed, restated: what the defaults must still give"""
    per = N_rand // N_images
    picks = ds.rng.choice(len(ds), size=N_images, replace=len(ds) < N_images)
    pixels = [ds.rng.choice(ds.sampling_idxs[i], size=per, replace=len(ds.sampling_idxs[i]) < per) for i in picks]
    lo, hi = rank * N_images // world, (rank + 1) * N_images // world
    out = {k: [] for k in ref.KEYS}
    for i, pix in list(zip(picks, pixels))[lo:hi]:
        ro, rd = ds._rays(i, pix)
        out["rays_o"].append(ro), out["rays_d"].append(rd)
        out["target_s"].append(ds.imgs[i].reshape(-1, 3)[pix])
        out["fgs"].append(ds.fgs[i].reshape(-1, 1)[pix])
        out["bgs"].append(ds.bgs[ds.bg_idxs[i]].reshape(-1, 3)[pix])
        for k, src in (("kp3d", ds.kp3d), ("bones", ds.bones), ("skts", ds.skts), ("cyls", ds.cyls)):
            out[k].append(np.broadcast_to(src[i], (per,) + src[i].shape))
        out["cam_idxs"].append(np.full(per, ds.cam_idxs[i])), out["kp_idx"].append(np.full(per, i))
    batch = {k: torch.tensor(np.concatenate(v)) for k, v in out.items()}
    batch["N_uniques"] = hi - lo
    return batch


@pytest.mark.parametrize("centers", [None, "f32"])
def test_defaults_give_the_batches_of_before(centers):
    a, b, c = ref.toy_dataset(centers), ref.toy_dataset(centers, mask_image=False, perturb_bg=False, sampling_masks=None), ref.toy_dataset(centers)
    assert not a.mask_image and not a.perturb_bg and not a.mask_sampling
    for n_images, n_rand in ref.MATRIX + [(4, 64)]:
        x = a.sample_batch(n_images, n_rand)
        assert batches_equal(x, b.sample_batch(n_images, n_rand)) and batches_equal(x, parent_sample_batch(c, n_images, n_rand))
    assert a.rng.bit_generator.state == b.rng.bit_generator.state == c.rng.bit_generator.state
    for rank in (0, 1):
        assert batches_equal(a.sample_batch(4, 64, rank, 2), parent_sample_batch(c, 4, 64, rank, 2))
    assert a.rng.bit_generator.state == c.rng.bit_generator.state


@pytest.mark.parametrize("flags", FLAGS[1:])
def test_flags_leave_the_rays_alone(flags):
    off, on = ref.toy_dataset("f32"), ref.toy_dataset("f32", **flags)
    for _ in range(3):                                   # (the noise is drawn after the pixels: later batches differ in their draws)
        a, b = off.sample_batch(4, 64), on.sample_batch(4, 64)
        assert all(ref.same_bits(a[k].numpy(), b[k].numpy()) for k in ("rays_o", "rays_d", "kp_idx", "cam_idxs", "fgs", "skts"))
        if flags.get("perturb_bg"):
            off.rng.random((64, 3), dtype=np.float32)    # the generators are in step again


@pytest.mark.parametrize("flags", FLAGS)
def test_targets_and_backgrounds_are_the_two_formulas(flags):
    ds, twin = ref.toy_dataset(**flags), ref.toy_dataset(**flags)
    some_fraction = False
    for rank, world in ((0, 1), (0, 2), (1, 2)):
        b = ds.sample_batch(4, 64, rank, world)
        per, picks, pixels, noise = twin._draw(4, 64, rank, world)
        assert (noise is not None) == bool(flags.get("perturb_bg")) and len(picks) == 4 // world == b["N_uniques"]
        one = np.float32(1)
        for n, (i, pix) in enumerate(zip(picks, pixels)):
            fg, img, bg = ds.fgs[i].reshape(-1, 1)[pix], ds.imgs[i].reshape(-1, 3)[pix], ds.bgs[ds.bg_idxs[i]].reshape(-1, 3)[pix]
            if flags.get("perturb_bg"):
                bg = (one - fg) * noise[n * per:(n + 1) * per] + fg * bg
            if flags.get("mask_image"):
                img = img * fg + (one - fg) * bg
            rows = slice(n * per, (n + 1) * per)
            assert img.dtype == bg.dtype == np.float32
            assert ref.same_bits(b["target_s"][rows].numpy(), img) and ref.same_bits(b["bgs"][rows].numpy(), bg)
            assert ref.same_bits(b["fgs"][rows].numpy(), fg)
            some_fraction |= bool(np.any(fg == 0.25))
    assert some_fraction                                 # both formulas did arithmetic


def test_mask_image_changes_the_targets_outside_the_mask():
    """the test that fails without the feature: the flag-free twin's targets are the stored colours imgs[i][pix]"""
    b = ref.toy_dataset(mask_image=True).sample_batch(4, 64)
    plain = ref.toy_dataset().sample_batch(4, 64)
    fg = b["fgs"].numpy()[:, 0]
    assert ref.same_bits(plain["fgs"].numpy(), b["fgs"].numpy())
    same = (b["target_s"].numpy() == plain["target_s"].numpy()).all(-1)
    assert (fg < 1).any() and (fg == 1).any()
    assert not same[fg < 1].any() and same[fg == 1].all()


def test_sampling_masks_choose_the_pixels():
    masks = np.zeros((6, H, W), np.uint8)
    masks[:, 3:9, 5:12] = 7                              # 42 pixels: enough for 16 a draw
    masks[1] = 0                                         # empty
    masks[2] = 0
    masks[2, 5, 5:12] = 1                                # 7 pixels: fewer than a draw takes
    ds = ref.toy_dataset(sampling_masks=masks)
    assert ds.mask_sampling and [len(s) for s in ds.sampling_idxs] == [42, 0, 7, 42, 42, 42]
    seen = set()
    for _ in range(12):
        per, picks, pixels, _ = ds._draw(4, 64, 0, 1)
        for i, pix in zip(picks, pixels):
            assert len(pix) == per == 16 and len(set(pix.tolist())) == 16          # never a repeat
            assert 0 <= pix.min() and pix.max() < H * W
            if i in (1, 2):
                seen.add(int(i))
                assert not masks[i].reshape(-1)[pix].all()                         # the whole image, not the 0 / 7 pixels
            else:
                assert masks[i].reshape(-1)[pix].all()
    assert seen == {1, 2}
    with pytest.raises(ValueError, match="sampling_masks"):
        ref.toy_dataset(sampling_masks=masks[:, :8])
    # float masks, any dtype: > 0 is what counts
    ds = ref.toy_dataset(sampling_masks=np.where(masks > 0, 0.5, -1.0))
    assert [len(s) for s in ds.sampling_idxs] == [42, 0, 7, 42, 42, 42]


# ----------------------------------------------------------------------------- the serial restatement
@pytest.mark.parametrize("n_images, n_rand", ref.MATRIX)
@pytest.mark.parametrize("centers", [None, "f32"])
def test_restatement_equals_the_numpy_path_bit_for_bit(centers, n_images, n_rand):
    """float32 centres only: a float64 `centers` array makes numpy's host path compute the directions in float64 (and return
    float64 rays), which is not what the device computes from the float32 centres it is given"""
    for flags in (FLAGS[0], FLAGS[3]):
        for rank, world in ((0, 1), (0, 2), (1, 2)):
            if n_images % world:
                continue
            ds, twin = ref.toy_dataset(centers, seed=3, **flags), ref.toy_dataset(centers, seed=3, **flags)
            for _ in range(2):
                want = ds.sample_batch(n_images, n_rand, rank, world)
                per, picks, pixels, noise = ref.draw(twin, n_images, n_rand, rank, world)
                got = ref.host_gather(ref.tables_of(twin), H, W, per, picks, pixels, noise, twin.mask_image)
                for k in ref.KEYS:
                    assert ref.same_bits(got[k], want[k].numpy()), (k, flags, rank, world)
                assert want["N_uniques"] == len(picks)


def test_restatement_clamps_what_it_cannot_trust():
    ds = ref.toy_dataset("f32", mask_image=True, perturb_bg=True)
    tab = ref.tables_of(ds)
    noise = np.random.default_rng(1).random((12, 3), dtype=np.float32)
    picks = np.array([-3, 99, 2, 2 ** 31 - 1], np.int32)
    pixels = np.array([-1, H * W, 5, H * W + 5, 2 ** 31 - 1, -2 ** 31, 0, H * W - 1, 17, 319, 320, -7], np.int32)
    bad = dict(tab, bg_idxs=np.array([7, -2, 1, 0, 2 ** 31 - 1, -2 ** 31], np.int32))
    got = ref.host_gather(bad, H, W, 3, picks, pixels, noise, True)
    want = ref.host_gather(dict(tab, bg_idxs=np.clip(bad["bg_idxs"], 0, 1)), H, W, 3, np.clip(picks, 0, 5), np.clip(pixels, 0, H * W - 1),
                           noise, True)
    assert all(ref.same_bits(got[k], want[k]) for k in ref.KEYS)
    assert got["kp_idx"].tolist() == [0] * 3 + [5] * 3 + [2] * 3 + [5] * 3


# ----------------------------------------------------------------------------- the header and its binding
def test_header_is_a_satellite_of_the_table():
    """what tests/test_abi_binding.py's referee does not hold: the host restatement is typed as the header types the entry"""
    from core import _hip
    assert "danbo_batch.h" in _hip.HEADERS
    h = _hip.header("danbo_batch.h")
    assert os.path.samefile(h.path, os.path.join(ROOT, "include", "danbo_batch.h"))
    assert h.signatures["danbo_batch_gather"] == ref.ARGTYPES + [ctypes.c_void_p] and h.restypes["danbo_batch_gather"] is ctypes.c_int


# ----------------------------------------------------------------------------- argument checks (no GPU: nothing is launched)
_NAMES = ["imgs", "fgs", "bgs", "bg_idxs", "cam_idxs", "c2ws", "focals", "centers", "kp3d", "bones", "skts", "cyls", "N", "B", "H", "W",
          "picks", "pixels", "noise", "G", "per", "mask_image"] + ["o_" + k for k in ref.KEYS]


def batch_gather(**kw):
    a = {k: P for k in _NAMES}
    a.update(N=6, B=2, H=16, W=20, G=4, per=16, mask_image=1)
    assert set(kw) <= set(a)
    a.update(kw)
    return entry("danbo_batch_gather")(*(a[k] for k in _NAMES), None)


@pytest.mark.parametrize("kw", [{k: None} for k in _NAMES if k not in ("centers", "noise", "N", "B", "H", "W", "G", "per", "mask_image")]
                         + [dict(N=0), dict(B=0), dict(H=0), dict(W=0), dict(per=0), dict(N=-1), dict(per=-4), dict(G=-1),
                            dict(H=65536, W=32768), dict(G=65536, per=32768), dict(G=2 ** 31 - 1, per=2)],
                         ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_batch_gather_rejects_before_any_launch(kw):
    assert batch_gather(**kw) == EINVAL


def test_batch_gather_of_no_picks_launches_nothing():
    assert batch_gather(G=0) == 0
    assert batch_gather(G=0, centers=None, noise=None, mask_image=0) == 0


def test_device_path_refuses_without_tables_and_checks_the_draw():
    ds = ref.toy_dataset()
    with pytest.raises(RuntimeError, match="to_device"):
        ds.sample_batch(4, 64, on_device=True)
    with pytest.raises(RuntimeError, match="no GPU"):
        ds.to_device("cpu")
    ds.sampling_idxs = [np.array([H * W + 3])] * 6
    with pytest.raises(ValueError, match="pixel indices"):
        ds.sample_batch(4, 64, on_device=True)
    ds.sampling_idxs = [np.array([-1])] * 6
    with pytest.raises(ValueError, match="pixel indices"):
        ds.sample_batch(4, 64, on_device=True)


# ----------------------------------------------------------------------------- flags
def test_flags_parse_from_argv_and_from_a_config_text(tmp_path):
    from core.config import config_parser, parse_args
    a = config_parser().parse_args([])
    assert (a.mask_image, a.perturb_bg, a.device_data) == (False, False, False)
    a = parse_args(["--mask_image", "--perturb_bg", "--device_data"])
    assert (a.mask_image, a.perturb_bg, a.device_data) == (True, True, True)
    cfg = tmp_path / "ref.txt"
    cfg.write_text("expname = x\nmask_image = True\nperturb_bg = True\nN_rand = 64\n")
    a = parse_args([], config=str(cfg))
    assert (a.mask_image, a.perturb_bg, a.device_data, a.N_rand) == (True, True, False, 64)
    cfg.write_text("mask_image = False\n")
    assert parse_args([], config=str(cfg)).mask_image is False


def test_load_data_passes_the_flags_and_device_data_needs_a_gpu():
    from core.config import parse_args
    from core.load_data import load_data
    images = (np.zeros((4, 16, 16, 3), np.float32), np.zeros((4, 16, 16, 1), np.float32))
    base = ["--syn_poses", "2", "--syn_cams", "2", "--syn_res", "16", "--N_sample_images", "2", "--N_rand", "8"]
    it, _, _ = load_data(parse_args(base + ["--mask_image", "--perturb_bg"]), images=images)
    ds = it.gi_frame.f_locals["dataset"]
    assert ds.mask_image and ds.perturb_bg and ds._device is None
    it, _, _ = load_data(parse_args(base), images=images)
    assert not it.gi_frame.f_locals["dataset"].mask_image and not it.gi_frame.f_locals["dataset"].perturb_bg
    with pytest.raises(RuntimeError, match="no GPU visible"):
        load_data(parse_args(base + ["--device_data"]), device=torch.device("cpu"), images=images)
