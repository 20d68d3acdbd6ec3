"""Helpers of the image-metrics tests (tests/test_image_metrics_host.py, tests/test_gpu_image_metrics.py): the serial restatement
of csrc/metrics_math.hpp built with g++ at test time, a float64 numpy evaluation of the crop-then-zero-pad SSIM and the squared
error, and the textured test frames."""
import ctypes
import os

import numpy as np

import hostlib
import mesh_ref
from helpers import ROOT

F32 = np.float32
CSRC = os.path.join(ROOT, "danbo-pytorch_amd", "csrc")
N_SUMS = 8
# the bounds of the issue: SSIM means 2e-5 (the map bound of test_ssim_map_known_answer) + < 1e-5 for ~22 tree levels of 2^-24;
# PSNR (10 / ln 10) x ~1.5e-6 relative error of the sum, rounded up to the bound test_psnr_ssim_identities uses
MAP_TOL, SSIM_TOL, PSNR_TOL = 2e-5, 3e-5, 1e-4

_WRAPPER = '''#include "%s"
using namespace danbo;
extern "C" {
size_t ref_metrics_workspace_bytes(int n_images, int height, int width) { return metrics_workspace_size(n_images, height, width); }
int ref_image_metrics(const float* pred, const float* gt, const float* mask_a, const float* mask_b, const int32_t* boxes, int n_images,
                      int height, int width, const float* window, int win, void* workspace, float* sums, float* ssim_map) {
    return image_metrics_host(pred, gt, mask_a, mask_b, boxes, n_images, height, width, window, win, workspace, sums, ssim_map);
}
int ref_tile_h(void) { return METRICS_TILE_H; }
int ref_tile_w(void) { return METRICS_TILE_W; }
}
'''


def host_lib():
    """g++ -O2 -std=c++17 -ffp-contract=off build of the serial restatement (csrc/metrics_math.hpp)"""
    lib = hostlib.build("metrics_ref", _WRAPPER % os.path.join(CSRC, "metrics_math.hpp"))
    c = ctypes
    lib.ref_metrics_workspace_bytes.argtypes = [c.c_int] * 3
    lib.ref_metrics_workspace_bytes.restype = c.c_size_t
    lib.ref_image_metrics.argtypes = [c.c_void_p] * 5 + [c.c_int] * 3 + [c.c_void_p, c.c_int] + [c.c_void_p] * 3
    return lib


def tile():
    """(TILE_H, TILE_W) of csrc/metrics_math.hpp"""
    return host_lib().ref_tile_h(), host_lib().ref_tile_w()


def window(win=11, sigma=1.5):
    """the weights the product hands the kernel: evaluation_helpers._gauss as a float32 array"""
    from core.utils.evaluation_helpers import _gauss
    return _gauss(win, sigma).numpy().astype(F32)


def aligned(shape, dtype=F32, fill=0):
    """a 16-byte aligned array, as the C call wants pred, gt and ssim_map"""
    n = int(np.prod(shape))
    raw = np.zeros(n * np.dtype(dtype).itemsize + 16, np.uint8)
    off = (-raw.ctypes.data) % 16
    a = raw[off:off + n * np.dtype(dtype).itemsize].view(dtype).reshape(shape)
    a[...] = fill
    return a


def _al(a):
    a = np.ascontiguousarray(a, F32)
    if a.ctypes.data % 16:
        b = aligned(a.shape)
        b[...] = a
        a = b
    return a


MAP_FILL = F32(-7.5)          # what the map holds before the call: a pixel outside the box keeps it


def host_metrics(pred, gt, mask_a=None, mask_b=None, boxes=None, win=11, want_map=True, w=None):
    """The serial restatement -> (sums [N,8] float32, ssim_map [N,H,W,3] float32 or None); the map is pre-filled with MAP_FILL;
    guard words around the workspace and the sums are checked."""
    lib = host_lib()
    pred, gt = _al(pred), _al(gt)
    N, H, W = pred.shape[:3]
    assert pred.shape == gt.shape == (N, H, W, 3)
    ma = None if mask_a is None else np.ascontiguousarray(mask_a, F32).reshape(N, H, W)
    mb = None if mask_b is None else np.ascontiguousarray(mask_b, F32).reshape(N, H, W)
    bx = None if boxes is None else np.ascontiguousarray(boxes, np.int32).reshape(N, 4)
    w = window(win) if w is None else np.ascontiguousarray(w, F32)
    n_bytes = lib.ref_metrics_workspace_bytes(N, H, W)
    assert n_bytes > 0 and n_bytes % 4 == 0
    ws_buf, ws = mesh_ref.guarded(n_bytes // 4, F32)
    s_buf, sums = mesh_ref.guarded(max(N, 1) * N_SUMS, F32)
    m = None
    if want_map:
        m = aligned((N, H, W, 3), fill=MAP_FILL)
    p = lambda a: None if a is None else a.ctypes.data      # noqa: E731
    rc = lib.ref_image_metrics(p(pred), p(gt), p(ma), p(mb), p(bx), N, H, W, p(w), win, p(ws), p(sums), p(m))
    assert rc == 0, rc
    assert mesh_ref.guards_intact(ws_buf) and mesh_ref.guards_intact(s_buf), "a guard word was overwritten"
    return sums[:N * N_SUMS].reshape(N, N_SUMS).copy(), m


def clamp_box(box, H, W):
    x0, y0, x1, y1 = (int(v) for v in box)
    c = lambda v, hi: min(max(v, 0), hi)      # noqa: E731
    return c(x0, W), c(y0, H), c(x1, W), c(y1, H)


# ----------------------------------------------------------------------------- float64 evaluation
def _blur64(x, g):
    """x [H,W,C] float64, zero padded, first over H then over W"""
    p = len(g) // 2
    H, W = x.shape[:2]
    xp = np.pad(x, ((p, p), (0, 0), (0, 0)))
    x = sum(g[t] * xp[t:t + H] for t in range(len(g)))
    xp = np.pad(x, ((0, 0), (p, p), (0, 0)))
    return sum(g[t] * xp[:, t:t + W] for t in range(len(g)))


def ssim_f64(x, y, w=None):
    """per-pixel, per-channel SSIM of one [H,W,C] pair in float64, zero padding (the float32 window's weights, in float64)"""
    g = (window() if w is None else np.asarray(w)).astype(np.float64)
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    mu1, mu2 = _blur64(x, g), _blur64(y, g)
    s1, s2, s12 = _blur64(x * x, g) - mu1 * mu1, _blur64(y * y, g) - mu2 * mu2, _blur64(x * y, g) - mu1 * mu2
    return (2 * mu1 * mu2 + 1e-4) / (mu1 * mu1 + mu2 * mu2 + 1e-4) * ((2 * s12 + 9e-4) / (s1 + s2 + 9e-4))


def metrics_f64(pred, gt, mask_a=None, mask_b=None, boxes=None, w=None):
    """float64 sums [N,8] in the order of danbo_image_metrics, and the float64 map [N,H,W,3] (nan outside the boxes): the SSIM of
    each CROP, zero padded"""
    pred, gt = np.asarray(pred, np.float64), np.asarray(gt, np.float64)
    N, H, W = pred.shape[:3]
    sums, maps = np.zeros((N, N_SUMS)), np.full((N, H, W, 3), np.nan)
    for n in range(N):
        x0, y0, x1, y1 = clamp_box(boxes[n], H, W) if boxes is not None else (0, 0, W, H)
        if x1 <= x0 or y1 <= y0:
            continue
        sl = (n, slice(y0, y1), slice(x0, x1))
        s = ssim_f64(pred[sl], gt[sl], w)
        se = np.square(gt[sl] - pred[sl])
        maps[sl] = s
        sums[n, 0], sums[n, 1] = se.sum(), s.sum()
        for k, m in ((2, mask_a), (5, mask_b)):
            if m is not None:
                mm = np.asarray(m, np.float64).reshape(N, H, W)[sl][..., None]
                sums[n, k], sums[n, k + 1], sums[n, k + 2] = (se * mm).sum(), (s * mm).sum(), mm.sum()
    return sums, maps


def psnr(sum_se, count):
    """-10 log10 of a mean squared error from its sum and the number of values"""
    with np.errstate(divide="ignore"):
        return -10. * np.log10(np.asarray(sum_se, np.float64) / count)


def frames(seed, N, H, W, noise=0.08):
    """textured frames as the golden's: uniform noise as ground truth, a noisy clipped copy as the prediction -> pred, gt float32"""
    rng = np.random.default_rng(seed)
    gt = rng.uniform(size=(N, H, W, 3))
    pred = np.clip(gt + noise * rng.normal(size=gt.shape), 0, 1)
    return pred.astype(F32), gt.astype(F32)
