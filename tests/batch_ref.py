"""Helpers of the training-batch tests (tests/test_batch_host.py, tests/test_gpu_batch.py): the serial restatement of
csrc/batch_math.hpp (batch_gather_host) built with g++ at test time, and the toy data set both files draw from."""
import ctypes
import os

import numpy as np

import hostlib
import mesh_ref
from helpers import ROOT

F32 = np.float32
CSRC = os.path.join(ROOT, "danbo-pytorch_amd", "csrc")
KEYS = ("rays_o", "rays_d", "target_s", "fgs", "bgs", "kp3d", "bones", "skts", "cyls", "cam_idxs", "kp_idx")      # of sample_batch
TABLES = ("imgs", "fgs", "bgs", "bg_idxs", "cam_idxs", "c2ws", "focals", "centers", "kp3d", "bones", "skts", "cyls")  # C order
ROWS = dict(rays_o=(3,), rays_d=(3,), target_s=(3,), fgs=(1,), bgs=(3,), kp3d=(24, 3), bones=(24, 3), skts=(24, 4, 4), cyls=(5,),
            cam_idxs=(), kp_idx=())
# (N_images, N_rand) of the issue: (8, 64) draws more images than the toy set has, so images repeat; (4, 20): 5 rays an image
MATRIX = [(4, 64), (4, 20), (8, 64), (1, 1)]

_PARAMS = ("const float* imgs, const float* fgs, const float* bgs, const int32_t* bg_idxs, const int32_t* cam_idxs, const float* c2ws, "
           "const float* focals, const float* centers, const float* kp3d, const float* bones, const float* skts, const float* cyls, "
           "int n_images, int n_bgs, int height, int width, const int32_t* picks, const int32_t* pixels, const float* noise, "
           "int n_picks, int per, int mask_image, float* o_rays_o, float* o_rays_d, float* o_target, float* o_fgs, float* o_bgs, "
           "float* o_kp3d, float* o_bones, float* o_skts, float* o_cyls, long long* o_cam_idxs, long long* o_kp_idx")
_WRAPPER = '''#include "%s"
using namespace danbo;
extern "C" int ref_batch_gather(''' + _PARAMS + ''') {
    const BatchTables t = {imgs, fgs, bgs, bg_idxs, cam_idxs, c2ws, focals, centers, kp3d, bones, skts, cyls, n_images, n_bgs, height, width};
    const BatchDraw d = {picks, pixels, noise, n_picks, per, mask_image};
    const BatchOut out = {o_rays_o, o_rays_d, o_target, o_fgs, o_bgs, o_kp3d, o_bones, o_skts, o_cyls, o_cam_idxs, o_kp_idx};
    return batch_gather_host(t, d, out);
}
'''
ARGTYPES = [ctypes.c_void_p] * 12 + [ctypes.c_int] * 4 + [ctypes.c_void_p] * 3 + [ctypes.c_int] * 3 + [ctypes.c_void_p] * 11


def host_lib():
    """g++ -O2 -std=c++17 -ffp-contract=off build of the serial restatement (csrc/batch_math.hpp)"""
    lib = hostlib.build("batch_ref", _WRAPPER % os.path.join(CSRC, "batch_math.hpp"))
    lib.ref_batch_gather.argtypes = ARGTYPES
    return lib


# ----------------------------------------------------------------------------- the toy data set
def toy_arrays(centers=None, n=6, H=16, W=20):
    """the construction of tests/test_entry_points.py::_toy_dataset with two different backgrounds, fractional masks and a
    permutation as camera indices -> keyword arguments of PoseImageDataset; centers: None or "f32" (float32, off the middle)"""
    from core.load_data import synthetic_arrays
    arr = synthetic_arrays(n_poses=3, n_cams=2, H=H, W=W, pose_seed=1)
    rng = np.random.default_rng(0)
    imgs = rng.uniform(size=(n, H, W, 3)).astype(F32)
    fgs = np.zeros((n, H, W, 1), F32)
    fgs[:, 2:14, 4:16] = 0.25
    fgs[:, 4:12, 6:14] = 1
    bgs = rng.uniform(size=(2, H, W, 3)).astype(F32)
    kw = dict(imgs=imgs, fgs=fgs, bgs=bgs, bg_idxs=np.array([0, 1, 1, 0, 1, 0]), c2ws=arr["c2ws"], focals=arr["focals"],
              kp3d=arr["kp3d"], bones=arr["bones"], skts=arr["skts"], rest_pose=arr["rest_pose"], cam_idxs=np.array([3, 0, 5, 1, 4, 2]))
    if centers == "f32":
        kw["centers"] = (np.array([W * 0.5, H * 0.5]) + rng.uniform(-2.5, 2.5, size=(n, 2))).astype(F32)
    else:
        assert centers is None
    return kw


def toy_dataset(centers=None, seed=0, **flags):
    from core.load_data import PoseImageDataset
    return PoseImageDataset(**toy_arrays(centers), seed=seed, **flags)


def tables_of(ds):
    """the tables of a data set as to_device() uploads them: contiguous, indices int32, centers float32 or None"""
    t = {k: np.ascontiguousarray(getattr(ds, k)) for k in TABLES if k != "centers"}
    t["bg_idxs"], t["cam_idxs"] = t["bg_idxs"].astype(np.int32), t["cam_idxs"].astype(np.int32)
    t["centers"] = None if ds.centers is None else np.ascontiguousarray(ds.centers, F32)
    return t


def draw(ds, N_images, N_rand, rank=0, world=1):
    """the next draw of a data set's generator, as the C entry takes it -> per, picks int32 [G], pixels int32 [G*per], noise or None"""
    per, picks, pixels, noise = ds._draw(N_images, N_rand, rank, world)
    return per, picks.astype(np.int32), np.concatenate(pixels).astype(np.int32), None if noise is None else np.ascontiguousarray(noise)


def host_gather(tables, H, W, per, picks, pixels, noise, mask_image):
    """The serial restatement -> {key: array} in the shapes and types of sample_batch; guard words around every output checked."""
    G, R = len(picks), len(picks) * per
    out, bufs = {}, []
    for k in KEYS:
        n = max(R * int(np.prod(ROWS[k], dtype=np.int64)), 1)
        idx = k in ("cam_idxs", "kp_idx")
        buf, view = mesh_ref.guarded(2 * n if idx else n, np.int64 if idx else F32)
        bufs.append(buf)
        out[k] = view
    p = lambda a: None if a is None else a.ctypes.data      # noqa: E731
    picks, pixels = np.ascontiguousarray(picks, np.int32), np.ascontiguousarray(pixels, np.int32)
    noise = None if noise is None else np.ascontiguousarray(noise, F32)
    rc = host_lib().ref_batch_gather(*(p(tables[k]) for k in TABLES), len(tables["imgs"]), len(tables["bgs"]), H, W, p(picks), p(pixels),
                                     p(noise), G, per, int(mask_image), *(p(out[k]) for k in KEYS))
    assert rc == 0, rc
    assert all(mesh_ref.guards_intact(b) for b in bufs), "a guard word was overwritten"
    return {k: out[k][:R * int(np.prod(ROWS[k], dtype=np.int64))].reshape((R,) + ROWS[k]).copy() for k in KEYS}


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
