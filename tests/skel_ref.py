"""Helpers of the skeleton-overlay tests (tests/test_skel_host.py, tests/test_gpu_skel.py): an independent restatement of the
definitions of csrc/skel_math.hpp -- numpy float32 for the projection, Python integers (exact at any size) for the coverage rule and
the paint order --, the serial restatement of the header itself (skel_project_host / skel_draw_host) built with g++ at test time,
and the named cases."""
import ctypes
import functools
import os

import numpy as np

import hostlib
from helpers import ROOT

F32 = np.float32
CSRC = os.path.join(ROOT, "danbo-pytorch_amd", "csrc")
J = 24
SKIP = -2 ** 31
LIMIT = 2 ** 30
WIDTHS = (1, 2, 3, 8)

_WRAPPER = '''#include "%s"
using namespace danbo;
extern "C" {
int ref_skel_project(const float* kps, const float* w2c, const float* focals, int focal_stride, const float* centers, int N, int H, int W,
                     int32_t* ends) {
    return skel_project_host(kps, w2c, focals, focal_stride, centers, N, H, W, ends);
}
int ref_skel_draw(const void* src, int src_is_float, const int32_t* ends, const uint8_t* colours, int width, int N, int H, int W,
                  uint8_t* dst) {
    return skel_draw_host(src, src_is_float, ends, colours, width, N, H, W, dst);
}
// the unrounded image points [N,24,2] of the same projection
void ref_skel_uv(const float* kps, const float* w2c, const float* focals, int focal_stride, const float* centers, int N, int H, int W,
                 float* uv) {
    for (int n = 0; n < N; ++n) {
        float fx, fy, ox, oy;
        skel_camera(focals, focal_stride, centers, n, H, W, &fx, &fy, &ox, &oy);
        for (int j = 0; j < J; ++j)
            skel_uv(kps + ((long)n * J + j) * 3, w2c + (long)n * 12, fx, fy, ox, oy, uv + ((long)n * J + j) * 2, uv + ((long)n * J + j) * 2 + 1);
    }
}
int ref_skel_parent(int j) { return skel_parent(j); }
int ref_skel_quant(float c) { return (int)skel_quant(c); }
// coverage without the bounding-box reject
int ref_skel_covers(const int32_t* e, int x, int y, int width) { return skel_covers(skel_segment(e, width), x, y, width) ? 1 : 0; }
int ref_skel_in_box(const int32_t* e, int x, int y, int width) { return skel_in_box(skel_segment(e, width), x, y) ? 1 : 0; }
}
'''
_c = ctypes
PROJECT_ARGTYPES = [_c.c_void_p] * 3 + [_c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p]
DRAW_ARGTYPES = [_c.c_void_p, _c.c_int, _c.c_void_p, _c.c_void_p] + [_c.c_int] * 4 + [_c.c_void_p]


def host_lib():
    """g++ -O2 -std=c++17 -ffp-contract=off build of the serial restatement (csrc/skel_math.hpp)"""
    lib = hostlib.build("skel_ref", _WRAPPER % os.path.join(CSRC, "skel_math.hpp"))
    lib.ref_skel_project.argtypes = PROJECT_ARGTYPES
    lib.ref_skel_draw.argtypes = DRAW_ARGTYPES
    lib.ref_skel_uv.argtypes = PROJECT_ARGTYPES
    lib.ref_skel_uv.restype = None
    lib.ref_skel_quant.argtypes = [_c.c_float]
    lib.ref_skel_covers.argtypes = lib.ref_skel_in_box.argtypes = [_c.c_void_p, _c.c_int, _c.c_int, _c.c_int]
    return lib


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ----------------------------------------------------------------------------- the header's restatement, called
def _project_args(kps, w2c, focals, centers, H, W):
    kps, w2c, focals = (np.ascontiguousarray(a, F32) for a in (kps, w2c, focals))
    centers = None if centers is None else np.ascontiguousarray(centers, F32)
    N = len(kps)
    assert kps.shape == (N, J, 3) and w2c.shape == (N, 3, 4) and focals.shape in ((N, 1), (N, 2))
    keep = (kps, w2c, focals, centers)
    return keep, (kps.ctypes.data, w2c.ctypes.data, focals.ctypes.data, focals.shape[1], None if centers is None else centers.ctypes.data,
                  N, int(H), int(W))


def host_project(kps, w2c, focals, centers, H, W):
    """skel_project_host -> ends [N,24,4] int32"""
    keep, args = _project_args(kps, w2c, focals, centers, H, W)
    ends = np.full((len(kps), J, 4), 7, np.int32)
    rc = host_lib().ref_skel_project(*args, ends.ctypes.data)
    assert rc == 0, rc
    return ends


def host_uv(kps, w2c, focals, centers, H, W):
    """the unrounded image points of the header's projection -> [N,24,2] float32"""
    keep, args = _project_args(kps, w2c, focals, centers, H, W)
    uv = np.zeros((len(kps), J, 2), F32)
    host_lib().ref_skel_uv(*args, uv.ctypes.data)
    return uv


def host_draw(src, ends, colours, width, rc_only=False):
    """skel_draw_host -> [N,H,W,3] uint8"""
    src = np.ascontiguousarray(src)
    ends, colours = np.ascontiguousarray(ends, np.int32), np.ascontiguousarray(colours, np.uint8)
    N, H, W, _ = src.shape
    assert src.dtype in (F32, np.uint8) and ends.shape == (N, J, 4) and colours.shape == (J, 3)
    dst = np.full((N, H, W, 3), 0x5A, np.uint8)
    rc = host_lib().ref_skel_draw(src.ctypes.data, int(src.dtype == F32), ends.ctypes.data, colours.ctypes.data, int(width), N, H, W,
                                  dst.ctypes.data)
    if rc_only:
        return rc
    assert rc == 0, rc
    return dst


# ----------------------------------------------------------------------------- the independent restatement
def colours(flip=False):
    """[24,3] uint8 by the reference's rule on the joints' names"""
    from core.utils.synthetic import JOINT_NAMES
    table = {"left": ((100, 149, 237), (0, 128, 128)), "right": ((255, 0, 0), (128, 128, 0)), "": ((46, 204, 13), (128, 0, 128))}
    key = lambda n: "left" if "left" in n else "right" if "right" in n else ""      # noqa: E731
    return np.array([table[key(n)][int(bool(flip))] for n in JOINT_NAMES], np.uint8)


def parents():
    from core.utils.synthetic import JOINT_TREES
    return [int(p) for p in JOINT_TREES]


def project_uv(kps, w2c, focals, centers, H, W):
    """numpy float32, one operation after the other -> u, v [N,24] float32"""
    kps, E, focals = np.asarray(kps, F32), np.asarray(w2c, F32), np.asarray(focals, F32)
    N = len(kps)
    with np.errstate(all="ignore"):
        p = [kps[:, :, i] for i in range(3)]
        cam = [((E[:, r, 0, None] * p[0] + E[:, r, 1, None] * p[1]) + E[:, r, 2, None] * p[2]) + E[:, r, 3, None] for r in range(3)]
        zz = cam[2] + F32(1e-8)
        fx, fy = focals[:, 0, None], focals[:, -1, None]
        if centers is None:
            ox, oy = np.full((N, 1), F32(0.5) * F32(W), F32), np.full((N, 1), F32(0.5) * F32(H), F32)
        else:
            ox, oy = np.asarray(centers, F32)[:, 0, None], np.asarray(centers, F32)[:, 1, None]
        qu, qv = (fx * cam[0]) / zz, (fy * cam[1]) / zz
        qu[qu == np.inf] = 0
        qv[qv == np.inf] = 0
        u, v = qu + ox, qv + oy
    assert u.dtype == v.dtype == F32
    return u, v


def _coordinate(c):
    """a float32 coordinate as a Python int: round to nearest-even, clamped; None for NaN and -inf"""
    c = float(c)
    if c != c or c == -np.inf:
        return None
    if c == np.inf:
        return LIMIT
    return max(-LIMIT, min(LIMIT, round(c)))


def ends_from_uv(u, v):
    """-> ends [N,24,4] int32 by the rule of draw_skeleton2d"""
    par = parents()
    ends = np.zeros(u.shape + (4,), np.int32)
    with np.errstate(all="ignore"):
        for n in range(u.shape[0]):
            for j in range(J):
                uj, vj, up, vp = u[n, j], v[n, j], u[n, par[j]], v[n, par[j]]
                e = [_coordinate(c) for c in (uj, vj, uj + (up - uj), vj + (vp - vj))]
                ends[n, j] = [SKIP, 0, 0, 0] if None in e else e
    return ends


def covers(e, x, y, w):
    """the rule, in Python integers"""
    ax, ay, bx, by = (max(-LIMIT, min(LIMIT, int(c))) for c in e)
    dx, dy, rx, ry = bx - ax, by - ay, x - ax, y - ay
    L, t = dx * dx + dy * dy, rx * dx + ry * dy
    if t <= 0:
        return rx * rx + ry * ry <= (w * w) // 4
    if t >= L:
        return (x - bx) ** 2 + (y - by) ** 2 <= (w * w) // 4
    return (2 * abs(rx * dy - ry * dx)) ** 2 <= w * w * L


def bone_map(ends, H, W, w, reject=True):
    """-> [N,H,W] int8: the largest covering bone of every pixel, -1 for none.  reject: only the pixels of a segment's bounding box
    grown by ceil(w / 2) are asked (False: every pixel of the frame)"""
    out = np.full((len(ends), H, W), -1, np.int8)
    g = (w + 1) // 2
    for n, frame in enumerate(ends):
        for j, e in enumerate(frame):
            if int(e[0]) == SKIP:
                continue
            ax, ay, bx, by = (max(-LIMIT, min(LIMIT, int(c))) for c in e)
            xs = range(max(0, min(ax, bx) - g), min(W - 1, max(ax, bx) + g) + 1) if reject else range(W)
            ys = range(max(0, min(ay, by) - g), min(H - 1, max(ay, by) + g) + 1) if reject else range(H)
            for y in ys:
                for x in xs:
                    if covers(e, x, y, w):
                        out[n, y, x] = j
    return out


def quantise(src):
    """the uint8 frame of a source: a float32 one as (rgb * 255).astype(uint8) made total"""
    if src.dtype == np.uint8:
        return src.copy()
    with np.errstate(all="ignore"):
        s = np.asarray(src, F32) * F32(255)
        s = np.where(np.isnan(s), F32(0), s)
        return np.trunc(np.clip(s, F32(0), F32(255))).astype(np.uint8)


def paint(src, bones, table):
    """the overlay from a bone map"""
    out = quantise(src)
    hit = bones >= 0
    out[hit] = np.asarray(table, np.uint8)[bones[hit]]
    return out


def draw(src, ends, table, w):
    return paint(src, bone_map(ends, src.shape[1], src.shape[2], w), table)


# ----------------------------------------------------------------------------- cases
def rest_pose(scale=0.5):
    from core.utils.synthetic import SMPL_REST_POSE
    return (np.asarray(SMPL_REST_POSE, np.float64) * scale).astype(F32)


def ring_cameras(n, rng, dist=3.0):
    """c2w [n,4,4] float32 in the NeRF convention (the camera looks along its -z): on a ring about y, `dist` from the origin, with a
    small random tilt"""
    out = []
    for _ in range(n):
        th, ph = rng.uniform(0, 2 * np.pi), rng.uniform(-0.3, 0.3)
        ry = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]])
        rx = np.array([[1, 0, 0], [0, np.cos(ph), -np.sin(ph)], [0, np.sin(ph), np.cos(ph)]])
        R = ry @ rx
        c2w = np.eye(4)
        c2w[:3, :3], c2w[:3, 3] = R, R @ np.array([0, 0, dist])
        out.append(c2w)
    return np.array(out, F32)


def w2c_of(c2ws):
    from core.utils.skeleton_utils import nerf_c2w_to_extrinsic
    return np.array([nerf_c2w_to_extrinsic(c) for c in c2ws]).astype(F32)[:, :3, :]


IDENTITY_C2W = np.diag([1., -1., -1., 1.]).astype(F32)       # its world-to-camera matrix is the identity


def scene(N, H, W, seed, focal_stride=1, with_centers=False):
    """a jittered rest pose seen by ring cameras -> dict(kps, c2ws, focals [N,stride], centers, H, W)"""
    rng = np.random.default_rng(seed)
    kps = rest_pose()[None] + rng.normal(0, 0.03, (N, J, 3)).astype(F32)
    f = 1.1 * min(H, W)
    focals = (f * rng.uniform(0.9, 1.1, (N, focal_stride))).astype(F32)
    centers = (np.array([W / 2, H / 2]) + rng.uniform(-3, 3, (N, 2))).astype(F32) if with_centers else None
    return dict(kps=kps.astype(F32), c2ws=ring_cameras(N, rng), focals=focals, centers=centers, H=H, W=W)


def edge_scene(H=37, W=53):
    """three frames through the identity camera (x = px, y = py, z = pz): frame 0 a NaN and a -inf joint, frame 1 one joint behind
    the camera and one far outside the image, frame 2 quotients of +inf (-> 0), of -inf and 0 / 0"""
    kps = np.tile(rest_pose()[None], (3, 1, 1)).astype(F32)
    kps[..., 1] *= -1                  # image y grows downwards
    kps[..., 2] = 2.0
    kps[0, 5] = [np.nan, 0.1, 2.0]     # right knee: bones 5 and 8 (its child) are skipped
    kps[0, 18, 0] = -np.inf            # left elbow at x = -inf: u = -inf (and 0 * -inf = NaN in v), bones 18 and 20 are skipped
    kps[1, 15, 2] = -1.5               # head behind the camera
    kps[1, 22] = [40.0, -3.0, 2.0]     # left hand far to the right: one end outside the image
    kps[2, 10] = [1e30, 1e30, 1e-30]   # fx x / zz overflows: +inf -> 0 in both
    kps[2, 11] = [0.2, -0.2, -1e-8]    # zz = 0: +inf -> 0 in u, -inf in v -> skipped
    kps[2, 23] = [0.0, 0.1, -1e-8]     # 0 / 0 = NaN -> skipped
    c2ws = np.tile(IDENTITY_C2W[None], (3, 1, 1))
    focals = np.array([[24.0, 22.0], [25.0, 25.0], [20.0, 26.0]], F32)
    return dict(kps=kps, c2ws=c2ws, focals=focals, centers=None, H=H, W=W)


def _frame_of(segments):
    e = np.zeros((J, 4), np.int32)
    e[:, 0] = SKIP
    for j, seg in segments.items():
        e[j] = seg
    return e


def direct_ends():
    """ends that no projection made, for a 37 x 53 frame (H x W): frame 0 segments between ends at +-2^30 whose visible part
    crosses the frame (the 128-bit branch), frame 1 crossing bones, one end outside, a disc, frame 2 everything skipped but bone 23"""
    big = _frame_of({3: (-LIMIT, -LIMIT + 9, LIMIT - 9, LIMIT),                  # y = x + 9
                     7: (-LIMIT, -2 ** 29, LIMIT, 2 ** 29 + 30),                 # slope 1/2 through (0, 15)
                     12: (LIMIT, -LIMIT + 60, -LIMIT, LIMIT),                    # through (0, 30), a little flatter than -1, b left of a
                     20: (26, -LIMIT, 26, LIMIT)})                               # vertical
    cross = _frame_of({1: (2, 3, 50, 30), 2: (50, 3, 2, 30), 9: (-400, 18, 20, 18), 14: (30, 20, 30, 20), 0: (10, 30, 10, 30),
                       17: (45, -10, 60, 60), 21: (0, 0, 52, 36)})
    last = _frame_of({23: (5, 33, 48, 35)})
    return np.stack([big, cross, last])


# name -> the scene of a projection case
SCENES = {"1x5x7": lambda: scene(1, 5, 7, 1), "3x37x53": lambda: scene(3, 37, 53, 2, focal_stride=2, with_centers=True),
          "1x64x64": lambda: scene(1, 64, 64, 3, with_centers=True), "3x33x128": lambda: scene(3, 33, 128, 4, focal_stride=2),
          "edge": edge_scene}


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(kps, c2ws, w2c, focals, centers, H, W, ends): a scene and the restatement's ends (`direct`: ends alone)"""
    if name == "direct":
        c = dict(H=37, W=53, ends=direct_ends())
    else:
        c = SCENES[name]()
        c["w2c"] = w2c_of(c["c2ws"])
        c["ends"] = ends_from_uv(*project_uv(c["kps"], c["w2c"], c["focals"], c["centers"], c["H"], c["W"]))
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


CASES = tuple(SCENES) + ("direct",)
SPECIAL = np.array([0.0, 1.0, 0.999999, np.nan, -0.1, 1.5, -0.0, np.inf, -np.inf, 1e-30] +
                   [np.nextafter(F32(k / 255), F32(0)) for k in (1, 2, 127, 128, 254, 255)] + [k / 255 for k in (1, 128, 254)], F32)


@functools.lru_cache(maxsize=None)
def sources(name):
    """the float32 and the uint8 frames of a case -> (float [N,H,W,3], uint8 [N,H,W,3]); the float one holds the special values"""
    c = case(name)
    N, H, W = len(c["ends"]), c["H"], c["W"]
    rng = np.random.default_rng(H * 1000 + W)
    f = rng.random((N, H, W, 3), dtype=F32)
    flat = f.reshape(-1)
    flat[rng.choice(flat.size, len(SPECIAL), replace=False)] = SPECIAL
    u = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    f.setflags(write=False)
    u.setflags(write=False)
    return f, u


@functools.lru_cache(maxsize=None)
def bones_of(name, w):
    """the bone map of a case at width w, computed once"""
    c = case(name)
    m = bone_map(c["ends"], c["H"], c["W"], w)
    m.setflags(write=False)
    return m


def expected(name, w, is_float, flip=False):
    """the overlay of a case by the independent restatement"""
    return paint(sources(name)[0 if is_float else 1], bones_of(name, w), colours(flip))
