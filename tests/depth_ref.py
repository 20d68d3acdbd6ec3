"""Depth and normal maps (include/danbo_depth.h): what the tests of csrc/depth_math.hpp and csrc/k_depth.hip share.

  * the host build of the header's serial restatement (tests/hostlib.py), called through ctypes: host_composite / host_normals;
  * an independent statement of the same definitions in numpy float64 -- depth64, prefix64, level_accepts, normals64 -- written
    from the definitions, vectorised, sharing no code and no evaluation order with the header;
  * the cases both test files use, made once per process.

Bounds (u = 2^-24, the unit round-off of fp32; every input is an fp32 number, so the float64 statement reads exactly what the
fp32 code reads):
  expected depth   |depth - depth64| <= n u sum|w z|: n products and at most n - 1 + 6 additions lie on the path of any term
                   (its lane's chain of <= ceil(n / 64) additions, six tree steps), each with relative error <= u; first-order
                   (1 + u)^(n) - 1 ~ n u over the sum of the absolute terms.  The issue states this bound.
  level depth      the fp32 prefix of position k differs from the float64 prefix by at most n u (the weights are >= 0 and sum to
                   <= 1 here; at most n - 1 additions on any path), so the position the fp32 code finds is one whose float64 prefix is
                   >= level - n u while the float64 prefix of the position before it is < level + n u: the acceptance set of
                   level_accepts.  Near-ties need no exclusion.
  normals          normals64 returns the bound per pixel beside the colour, derived in its docstring.
"""
import ctypes
import functools
import os

import numpy as np

import hostlib
from helpers import ROOT

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
CSRC = os.path.join(ROOT, "danbo-pytorch_amd", "csrc")
MAX_N = 320
R_RAYS = 67
N_CASES = (1, 18, 64, 65, 320)       # one partial strip, (18: the S + Sf of the end-to-end frames), one full strip, one position into the
#                                      second strip, the limit
SENTINEL = F32(-777.25)

_WRAPPER = '''#include "%s"
using namespace danbo;
extern "C" {
int ref_depth_composite(const float* w, const float* z, int R, int n, float level, const int32_t* ray_list, const int32_t* ray_count,
                        float* depth, float* depth_level) {
    return depth_composite_host(w, z, R, n, level, ray_list, ray_count, depth, depth_level);
}
int ref_depth_normals(const float* depth, const float* acc, const uint8_t* cast, const float* c2w, const float* intr, int N, int H, int W,
                      float acc_min, float jump, int space, float background, float* out_rgb, uint8_t* out_valid) {
    return depth_normals_host(depth, acc, cast, c2w, intr, N, H, W, acc_min, jump, space, background, out_rgb, out_valid);
}
void ref_depth_wave_scan(float* x) { depth_wave_scan(x); }
}
'''
_c = ctypes
COMPOSITE_ARGTYPES = [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_float, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p]
NORMALS_ARGTYPES = [_c.c_void_p] * 5 + [_c.c_int] * 3 + [_c.c_float, _c.c_float, _c.c_int, _c.c_float, _c.c_void_p, _c.c_void_p]


def host_lib():
    """g++ -O2 -std=c++17 -ffp-contract=off build of the serial restatement (csrc/depth_math.hpp)"""
    lib = hostlib.build("depth_ref", _WRAPPER % os.path.join(CSRC, "depth_math.hpp"))
    lib.ref_depth_composite.argtypes = COMPOSITE_ARGTYPES
    lib.ref_depth_normals.argtypes = NORMALS_ARGTYPES
    lib.ref_depth_wave_scan.argtypes = [_c.c_void_p]
    lib.ref_depth_wave_scan.restype = None
    return lib


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ----------------------------------------------------------------------------- the header's restatement, called
def host_composite(w, z, level, ray_list=None, ray_count=None, init=None, rc_only=False):
    """-> (depth [R], depth_level [R]) of the restatement; init: what the outputs hold before the call (None: zeros)"""
    w, z = np.ascontiguousarray(w, F32), np.ascontiguousarray(z, F32)
    R, n = w.shape
    out = np.full((2, R), 0 if init is None else init, F32)
    lst = None if ray_list is None else np.ascontiguousarray(ray_list, np.int32)
    cnt = None if ray_count is None else np.array([ray_count], np.int32)
    rc = host_lib().ref_depth_composite(w.ctypes.data, z.ctypes.data, R, n, float(level), None if lst is None else lst.ctypes.data,
                                        None if cnt is None else cnt.ctypes.data, out[0].ctypes.data, out[1].ctypes.data)
    if rc_only:
        return rc
    assert rc == 0, rc
    return out[0], out[1]


def host_normals(depth, acc, cast, c2w, intr, acc_min=0.5, jump=0., space=0, background=1., rc_only=False):
    """-> (rgb [N,H,W,3] float32, valid [N,H,W] uint8) of the restatement"""
    depth, acc, c2w, intr = (np.ascontiguousarray(a, F32) for a in (depth, acc, c2w, intr))
    cast = None if cast is None else np.ascontiguousarray(cast, np.uint8)
    N, H, W = depth.shape
    rgb, valid = np.full((N, H, W, 3), np.nan, F32), np.full((N, H, W), 7, np.uint8)
    rc = host_lib().ref_depth_normals(depth.ctypes.data, acc.ctypes.data, None if cast is None else cast.ctypes.data, c2w.ctypes.data,
                                      intr.ctypes.data, N, H, W, float(acc_min), float(jump), int(space), float(background),
                                      rgb.ctypes.data, valid.ctypes.data)
    if rc_only:
        return rc
    assert rc == 0, rc
    return rgb, valid


def host_wave_scan(x):
    x = np.ascontiguousarray(x, F32).copy()
    assert x.shape == (64,)
    host_lib().ref_depth_wave_scan(x.ctypes.data)
    return x


# ----------------------------------------------------------------------------- float64, per ray
def depth64(w, z):
    """-> (sum_k w_k z_k [R], sum_k |w_k z_k| [R]) in float64; a position of weight 0 contributes 0 whatever z holds"""
    w, z = np.asarray(w, F64), np.asarray(z, F64)
    with np.errstate(invalid="ignore"):
        t = np.where(w == 0, 0.0, w * z)
    return t.sum(-1), np.abs(t).sum(-1)


def prefix64(w):
    return np.cumsum(np.asarray(w, F64), -1)


def level_accepts(got, w, z, level):
    """got [R] (fp32) against the acceptance set of every ray: z_k of a position k with prefix64[k] >= level - n u and
    prefix64[k - 1] < level + n u; +0 iff the total stays below level + n u.  -> list of the rays that are NOT accepted"""
    w, z = np.asarray(w, F32), np.asarray(z, F32)
    R, n = w.shape
    p, tol, bad = prefix64(w), n * U, []
    for r in range(R):
        before = np.concatenate([[0.0], p[r, :-1]])
        ok = (p[r] >= level - tol) & (before < level + tol)
        hit = any(same_bits(got[r], z[r, k]) for k in np.flatnonzero(ok))
        none = p[r, -1] < level + tol and same_bits(got[r], F32(0))
        if not (hit or none):
            bad.append(r)
    return bad


def depth_bound(w, z):
    """n u sum|w z| per ray (the issue's bound)"""
    return np.asarray(w).shape[1] * U * depth64(w, z)[1]


# ----------------------------------------------------------------------------- float64, per pixel
def _shift(a, dy, dx, fill):
    """out[n, y, x] = a[n, y + dy, x + dx], `fill` where that lies outside the frame"""
    out = np.full_like(a, fill)
    H, W = a.shape[1:3]
    ys, yd = slice(max(dy, 0), H + min(dy, 0)), slice(max(-dy, 0), H + min(-dy, 0))
    xs, xd = slice(max(dx, 0), W + min(dx, 0)), slice(max(-dx, 0), W + min(-dx, 0))
    out[:, yd, xd] = a[:, ys, xs]
    return out


def normals64(depth, acc, cast, c2w, intr, acc_min=0.5, jump=0., space=0, background=1.):
    """The normal map in float64, from the definitions (depth, acc of any float type; exact inputs give the exact map).
    -> (rgb [N,H,W,3], valid [N,H,W] bool, bound [N,H,W]): bound is what an fp32 evaluation of the same formulas may differ by in
    a colour channel, first-order terms doubled for the higher orders:
        D has one rounding, x - cx, the product and the quotient three more: every component of a point is within 4 u of its
        value, relatively, so |P^ - P| <= 4 u |P|;
        a difference d = Pa - Pb: e_d = 4 u (|Pa| + |Pb|) + u |d|                       (the cancellation: |d| ~ |P| / focal)
        the cross product c = dx x dy: e_c = e_dx |dy| + |dx| e_dy + 4 u |dx| |dy|      (inputs, then two products and a
                                                                                           difference per component)
        the unit normal: 2 e_c / |c| + 4 u (squares, sums, root, quotient); the rotation 6 u; the colour halves it and rounds
        twice more: 0.5 (2 e_c / |c| + 10 u) + 2 u, doubled:
        bound = 2 e_c / |c| + 14 u
    With |P| ~ D, |d| ~ D / focal and |c| ~ (D / focal)^2 the first term is ~ 32 u focal: proportional to focal 2^-24."""
    depth, acc = np.asarray(depth, F64), np.asarray(acc, F64)
    c2w, intr = np.asarray(c2w, F64), np.asarray(intr, F64)
    N, H, W = depth.shape
    with np.errstate(all="ignore"):
        D = depth / acc
        usable = (acc >= acc_min) & (D > 0)
    if cast is not None:
        usable &= np.asarray(cast) != 0
    D = np.where(usable, D, 0.0)
    fx, fy, cx, cy = (intr[:, i, None, None] for i in range(4))
    x, y = np.arange(W, dtype=F64)[None, None, :], np.arange(H, dtype=F64)[None, :, None]
    P = np.stack([D * (x - cx) / fx, -(D * (y - cy) / fy), -D + 0 * x], -1)
    norm = lambda v: np.sqrt((v * v).sum(-1))      # noqa: E731

    def difference(dy, dx):
        got = []
        for s in (-1, 1):
            ok = usable & _shift(usable, s * dy, s * dx, False)
            if jump > 0:
                ok &= np.abs(_shift(D, s * dy, s * dx, 0.0) - D) <= jump
            got.append((ok, _shift(P, s * dy, s * dx, 0.0)))
        (hb, Pb), (ha, Pa) = got
        both, only_a, only_b = (ha & hb)[..., None], (ha & ~hb)[..., None], (hb & ~ha)[..., None]
        d = np.where(both, Pa - Pb, np.where(only_a, Pa - P, np.where(only_b, P - Pb, 0.0)))
        ends = np.where(both[..., 0], norm(Pa) + norm(Pb), np.where(only_a[..., 0], norm(Pa) + norm(P), norm(P) + norm(Pb)))
        return d, ha | hb, 4 * U * ends + U * norm(d)

    dxv, hx, ex = difference(0, 1)
    dyv, hy, ey = difference(1, 0)
    c = np.cross(dxv, dyv)
    length = norm(c)
    valid = usable & hx & hy & (length > 0) & np.isfinite(length)
    with np.errstate(all="ignore"):
        n = c / length[..., None]
        n = np.where(((n * P).sum(-1) > 0)[..., None], -n, n)
        if space == 1:
            n = np.einsum("nij,nhwj->nhwi", c2w[:, :3, :3], n)
        e_c = ex * norm(dyv) + norm(dxv) * ey + 4 * U * norm(dxv) * norm(dyv)
        bound = np.where(valid, 2 * e_c / length + 14 * U, 0.0)
    rgb = np.where(valid[..., None], 0.5 * n + 0.5, float(background))
    return rgb, valid, bound


# ----------------------------------------------------------------------------- cases, per ray
@functools.lru_cache(maxsize=None)
def composite_case(n, seed=0):
    """R_RAYS rays of n positions: weights as a composite makes them (alpha (1 - alpha) products, sum <= 1) and ascending depths in
    [2, 5], with the special rays in front.  -> dict(w, z [R,n] float32, rays: name -> index)"""
    rng = np.random.default_rng(1000 * n + seed)
    R = R_RAYS
    alpha = rng.random((R, n)).astype(F32) * F32(0.2 if n > 64 else 0.6)
    alpha[rng.random((R, n)) < 0.3] = 0          # empty space between the surfaces
    trans = np.cumprod(np.concatenate([np.ones((R, 1), F32), (1 - alpha)[:, :-1]], 1, dtype=F32), 1, dtype=F32)
    w = (alpha * trans).astype(F32)
    z = np.sort(rng.uniform(2.0, 5.0, (R, n)).astype(F32), 1)
    for r in range(R):                           # strictly ascending: a depth names its position
        z[r] = F32(2.0) + np.arange(n, dtype=F32) * F32(3.0 / MAX_N) + (z[r] - F32(2.0)) * F32(1e-3)
    assert np.all(np.diff(z, axis=1) > 0) if n > 1 else True
    rays = {}
    rays["all_zero"] = 0                          # all weights +0
    w[0] = 0
    rays["below_level"] = 1                       # acc < 0.5: no position reaches the level
    w[1] = w[1] * F32(0.3) / max(F32(1e-3), w[1].sum(dtype=F32) * F32(1.25))
    rays["exact_tie"] = 2                         # the prefix equals the level exactly: 0.25 + 0.25 (n = 1: 0.5 alone)
    w[2] = 0
    if n == 1:
        w[2, 0] = 0.5
    else:
        w[2, n // 3], w[2, n // 3 + 1] = 0.25, 0.25
    rays["exact_one"] = 3                         # the weights sum to exactly 1: level = 1.0 is reached at the last of them
    w[3] = 0
    if n == 1:
        w[3, 0] = 1.0
    elif n == 2:
        w[3, :2] = 0.5
    else:
        w[3, 0], w[3, n // 2], w[3, n - 1] = 0.5, 0.25, 0.25
    rays["zero_weight_nan_depth"] = 4             # a position of weight +0 contributes +0 whatever its depth holds
    if n > 1:
        w[4, n // 2] = 0
        z[4, n // 2] = np.nan
    if n > 64:
        rays["tie_across_strips"] = 5             # 0.25 at the last lane of strip 0, 0.25 at the first of strip 1
        w[5] = 0
        w[5, 63], w[5, 64] = 0.25, 0.25
    assert w.dtype == F32 and z.dtype == F32 and np.all(w >= 0) and float(prefix64(w)[:, -1].max()) <= 1.0 + 1e-6
    w.setflags(write=False), z.setflags(write=False)
    return dict(w=w, z=z, rays=rays)


def tie_positions(n):
    """the two positions of composite_case's exact_tie ray"""
    return n // 3, n // 3 + 1


@functools.lru_cache(maxsize=None)
def composite_expected(n, level, seed=0):
    """the restatement's result on composite_case(n): computed once, shared, read-only"""
    c = composite_case(n, seed)
    d, l = host_composite(c["w"], c["z"], level)
    d.setflags(write=False), l.setflags(write=False)
    return d, l


@functools.lru_cache(maxsize=None)
def ray_list_case(n):
    """composite_case(n) with a list of 41 of its rays in a shuffled order (the special rays among them), the count, garbage
    beyond the count, and z rows that are NaN for every unlisted ray -> dict(w, z, ray_list [R], ray_count, listed [R] bool)"""
    c = composite_case(n)
    rng = np.random.default_rng(77 + n)
    order = rng.permutation(R_RAYS)
    special = sorted(c["rays"].values())
    rest = [r for r in order if r not in special]
    listed_rays = np.array(special + rest[:41 - len(special)], np.int32)
    rng.shuffle(listed_rays)
    lst = np.concatenate([listed_rays, np.array(rest[41 - len(special):], np.int32)])
    listed = np.zeros(R_RAYS, bool)
    listed[listed_rays] = True
    z = c["z"].copy()
    z[~listed] = np.nan
    z.setflags(write=False)
    return dict(w=c["w"], z=z, ray_list=lst.astype(np.int32), ray_count=41, listed=listed)


# ----------------------------------------------------------------------------- cases, per pixel
H_FRAME, W_FRAME = 9, 11
PLANE_NORMAL = np.array([0.3, -0.2, 0.9327379053088815])      # unit, facing the camera (z > 0)
PLANE_OFFSET = 3.0                                            # the plane {P : n . P = -PLANE_OFFSET}: 3 in front of the camera


def cameras(N=2):
    """c2w [N,3,4] (a rotation about y then x, and a translation) and intr [N,4] with fx != fy and off-centre, non-integer centres"""
    c2w, intr = np.zeros((N, 3, 4), F32), np.zeros((N, 4), F32)
    for i in range(N):
        a, b = 0.4 + 0.7 * i, -0.3 + 0.5 * i
        ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
        c2w[i, :, :3], c2w[i, :, 3] = ry @ rx, (0.1 * i, 1.0, 3.0 + i)
        intr[i] = (12.0 + i, 13.5 - i, 5.3 + 0.4 * i, 4.4 - 0.3 * i)
    return c2w, intr


def plane_depth(intr, normal=PLANE_NORMAL, offset=PLANE_OFFSET, H=H_FRAME, W=W_FRAME):
    """float64 [N,H,W]: the planar depth D at which the ray of every pixel meets the plane n . P = -offset (P = D r, r = ((x - cx)
    / fx, -(y - cy) / fy, -1))"""
    intr = np.asarray(intr, F64)
    x, y = np.arange(W, dtype=F64)[None, None, :], np.arange(H, dtype=F64)[None, :, None]
    r = np.stack([(x - intr[:, 2, None, None]) / intr[:, 0, None, None] + 0 * y, -(y - intr[:, 3, None, None]) / intr[:, 1, None, None] + 0 * x,
                  -np.ones((len(intr), H, W))], -1)
    return -offset / (r @ np.asarray(normal, F64))


@functools.lru_cache(maxsize=None)
def frames_case():
    """Two frames of 9 x 11.  Frame 0: the tilted plane under a varying opacity; frame 1: a curved surface with a step of 0.8 in
    depth down the middle (columns >= 6 lie behind).  Holes: pixels that were not cast, pixels of opacity 0 and pixels below the
    threshold 0.5 -- in the interior, on the border and in a corner; one usable pixel has no usable neighbour in its row.
    -> dict(depth, acc float32 [2,9,11], cast uint8, c2w, intr, D float64)"""
    rng = np.random.default_rng(5)
    c2w, intr = cameras(2)
    H, W = H_FRAME, W_FRAME
    D = plane_depth(intr)
    x, y = np.arange(W)[None, :], np.arange(H)[:, None]
    D[1] = 2.5 + 0.02 * (x - 5) ** 2 + 0.03 * (y - 4) + 0.8 * (x >= 6)
    acc = rng.uniform(0.6, 1.0, (2, H, W)).astype(F32)
    cast = np.ones((2, H, W), np.uint8)
    acc[0, 0, 0], acc[0, 4, 5], acc[1, 8, 10], acc[1, 3, 3] = 0.3, 0.3, 0.45, 0.0      # below the threshold / transparent
    acc[0, 8, 4] = 0.5                                                                   # exactly at the threshold: usable
    cast[0, 2, 7], cast[0, 0, 10], cast[1, 0, 5], cast[1, 5, 0] = 0, 0, 0, 0           # not cast: interior, corner, borders
    cast[1, 6, 7], cast[1, 6, 9] = 0, 0                                                 # (6, 8) of frame 1: no neighbour in its row
    cast[0, 6, 1], acc[0, 7, 0], cast[0, 8, 1] = 0, 0.1, 0                             # (7, 1) of frame 0: none in its column
    depth = (acc.astype(F64) * D).astype(F32)
    depth[cast == 0] = 0
    acc[cast == 0] = 0                                                                   # assembled like acc_img: 0 where not cast
    for a in (depth, acc, cast, c2w, intr, D):
        a.setflags(write=False)
    return dict(depth=depth, acc=acc, cast=cast, c2w=c2w, intr=intr, D=D)


NORMAL_VARIANTS = [dict(jump=0.0, space=0), dict(jump=0.0, space=1), dict(jump=0.4, space=0), dict(jump=0.4, space=1)]


@functools.lru_cache(maxsize=None)
def normals_expected(jump, space, with_cast=True):
    """the restatement's (rgb, valid) on frames_case(): computed once, shared, read-only"""
    c = frames_case()
    rgb, valid = host_normals(c["depth"], c["acc"], c["cast"] if with_cast else None, c["c2w"], c["intr"], 0.5, jump, space, 1.0)
    rgb.setflags(write=False), valid.setflags(write=False)
    return rgb, valid


# ----------------------------------------------------------------------------- rejected arguments (both test files)
PTR = "P"       # stands for a pointer the caller supplies: a host address no check follows, or a device buffer
_COMPOSITE = ["weights", "z_sorted", "R", "n", "level", "ray_list", "ray_count", "depth", "depth_level"]
_NORMALS = ["depth", "acc", "cast_mask", "c2w", "intr", "N", "H", "W", "acc_min", "jump", "space", "background", "out_rgb", "out_valid"]
COMPOSITE_REJECTS = [dict(weights=None), dict(z_sorted=None), dict(depth=None), dict(depth_level=None), dict(n=0), dict(n=321), dict(n=-1),
                     dict(R=-1), dict(level=0.0), dict(level=-0.5), dict(level=1.0000001), dict(level=float("nan")),
                     dict(ray_list=PTR), dict(ray_count=PTR)]
NORMALS_REJECTS = [dict(depth=None), dict(acc=None), dict(c2w=None), dict(intr=None), dict(out_rgb=None), dict(H=0), dict(H=4097),
                   dict(W=0), dict(W=4097), dict(N=0), dict(N=-2), dict(space=2), dict(space=-1), dict(jump=-0.5), dict(jump=float("nan"))]


def reject_id(kw):
    return "-".join(f"{k}={v}" for k, v in kw.items())


def _fill(names, base, kw, pointers):
    assert set(kw) <= set(base)
    a = dict(base, **kw)
    return [(pointers[k] if isinstance(pointers, dict) else pointers) if a[k] is PTR else a[k] for k in names]


def composite_args(pointers, **kw):
    """the arguments of the composite entry without the stream: a valid call (R = 4, n = 18) with `kw` laid over it; PTR becomes
    `pointers` (one address, or a dict name -> address)"""
    base = dict(weights=PTR, z_sorted=PTR, R=4, n=18, level=0.5, ray_list=None, ray_count=None, depth=PTR, depth_level=PTR)
    return _fill(_COMPOSITE, base, kw, pointers)


def normals_args(pointers, **kw):
    """likewise for the normals entry: one frame of 4 x 4"""
    base = dict(depth=PTR, acc=PTR, cast_mask=None, c2w=PTR, intr=PTR, N=1, H=4, W=4, acc_min=0.5, jump=0.0, space=0, background=1.0,
                out_rgb=PTR, out_valid=None)
    return _fill(_NORMALS, base, kw, pointers)
