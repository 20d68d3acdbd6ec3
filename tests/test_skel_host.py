"""The skeleton overlay (include/danbo_skel.h), the part that needs no GPU: the serial restatement of csrc/skel_math.hpp against the
independent one of tests/skel_ref.py (numpy float32, Python integers) bit for bit -- ends, skip marks and images --, the projection
against the reference's own functions, the properties of the coverage rule, the edge cases, the quantisation, the binding of the
header and the argument checks, which return before any launch."""
import ctypes
import os

import numpy as np
import pytest

import skel_ref as ref
from helpers import ADDR as P, EINVAL, ROOT, entry        # P: an address no check follows

F32 = np.float32
J, SKIP, LIMIT = ref.J, ref.SKIP, ref.LIMIT


def _ends(*segments):
    return np.array(segments, np.int32)


def c_covers(e, x, y, w):
    e = np.ascontiguousarray(e, np.int32)
    return bool(ref.host_lib().ref_skel_covers(e.ctypes.data, x, y, w))


# ----------------------------------------------------------------------------- the restatement against the independent one
def test_parent_table_is_the_skeletons():
    assert [ref.host_lib().ref_skel_parent(j) for j in range(J)] == ref.parents()
    assert ref.parents()[0] == 0            # the root's bone is the degenerate segment


@pytest.mark.parametrize("name", sorted(ref.SCENES))
def test_projection_equals_the_numpy_restatement(name):
    c = ref.case(name)
    args = (c["kps"], c["w2c"], c["focals"], c["centers"], c["H"], c["W"])
    u, v = ref.project_uv(*args)
    assert ref.same_bits(ref.host_uv(*args), np.stack([u, v], -1))
    got = ref.host_project(*args)
    assert ref.same_bits(got, c["ends"])
    skipped = got[..., 0] == SKIP
    assert np.all(got[skipped][:, 1:] == 0) and np.all(np.abs(got[~skipped].astype(np.int64)) <= LIMIT)
    # the root: a = b
    assert np.all((got[:, 0, :2] == got[:, 0, 2:]) | skipped[:, :1])


def test_edge_scene_skips_what_it_should():
    c = ref.case("edge")
    skipped = [np.flatnonzero(f[:, 0] == SKIP).tolist() for f in c["ends"]]
    # frame 0: the NaN knee (5) and its child (8), the -inf elbow (18) and its child (20); frame 2: -inf in v (11), 0 / 0 (23)
    assert skipped == [[5, 8, 18, 20], [], [11, 23]], skipped
    e = c["ends"]
    H, W = c["H"], c["W"]
    assert e[2, 10, :2].tolist() == [round(float(F32(0.5) * F32(W))), round(float(F32(0.5) * F32(H)))]          # +inf -> 0: the offset
    assert e[1, 22, 0] > 4 * W                       # one end far outside the image
    # the head behind the camera is mirrored through the centre, finite, and drawn
    assert e[1, 15, 0] != SKIP and e[1, 15, 1] > H / 2
    # and the rest of every frame is drawn
    for w in (1, 3):
        m = ref.bones_of("edge", w)
        assert all((m[n] >= 0).any() for n in range(3))
        assert not np.isin(m[0], [5, 8, 18, 20]).any() and not np.isin(m[2], [11, 23]).any()


@pytest.mark.parametrize("w", ref.WIDTHS)
@pytest.mark.parametrize("name", ref.CASES)
def test_draw_equals_the_integer_restatement(name, w):
    c = ref.case(name)
    for is_float in (True, False):
        src = ref.sources(name)[0 if is_float else 1]
        got = ref.host_draw(src, c["ends"], ref.colours(), w)
        want = ref.expected(name, w, is_float)
        assert ref.same_bits(got, want), (name, w, is_float, int((got != want).any(-1).sum()))
    flipped = ref.host_draw(ref.sources(name)[1], c["ends"], ref.colours(True), w)
    assert ref.same_bits(flipped, ref.expected(name, w, False, flip=True))
    if name != "1x5x7":
        assert (ref.bones_of(name, w) >= 0).any() and (ref.bones_of(name, w) < 0).any()


def test_colours_follow_the_joint_names():
    from core.utils.skeleton_draw import bone_colours
    from core.utils.synthetic import JOINT_NAMES
    for flip in (False, True):
        assert ref.same_bits(bone_colours(flip), ref.colours(flip))
    t = ref.colours()
    assert t[JOINT_NAMES.index("left_knee")].tolist() == [100, 149, 237] and t[JOINT_NAMES.index("right_hand")].tolist() == [255, 0, 0]
    assert t[0].tolist() == [46, 204, 13] and ref.colours(True)[0].tolist() == [128, 0, 128]
    assert len({tuple(r) for r in t}) == 3


def test_the_reject_changes_nothing():
    ends = ref.case("direct")["ends"]
    for w in (1, 8):
        assert ref.same_bits(ref.bone_map(ends, 37, 53, w, reject=False), ref.bones_of("direct", w))
    # the header's rule without its reject: whatever is covered lies in the box
    lib = ref.host_lib()
    for e in ends.reshape(-1, 4)[ends.reshape(-1, 4)[:, 0] != SKIP]:
        e = np.ascontiguousarray(e)
        for w in (1, 2, 7, 64):
            for y in range(0, 37):
                for x in range(0, 53):
                    cov = lib.ref_skel_covers(e.ctypes.data, x, y, w)
                    assert cov == int(ref.covers(e, x, y, w))
                    assert not cov or lib.ref_skel_in_box(e.ctypes.data, x, y, w)


# ----------------------------------------------------------------------------- the projection against the reference itself
REFERENCE_FUNCTIONS = ["swap_mat", "nerf_c2w_to_extrinsic", "coord_to_homogeneous", "focal_to_intrinsic_np", "world_to_cam", "skeleton3d_to_2d"]


@pytest.mark.parametrize("focal_stride, with_centers", [(1, False), (2, False), (1, True), (2, True)])
def test_projection_against_the_reference(focal_stride, with_centers):
    """The unrounded (u, v) of the restatement against the reference's skeleton3d_to_2d evaluated in float64, within 4 x delta,
    delta = the reference's own float32-against-float64 deviation on the same inputs (the margin covers the matrix product's
    unspecified summation order).  Eight ring cameras 3 units from a jittered rest pose at 512 x 512."""
    import ref_harness
    if not os.path.isfile(os.path.join(ref_harness.REF_ROOT, "core", "utils", "skeleton_utils.py")):
        pytest.skip("the reference tree is absent")
    fn = dict(zip(REFERENCE_FUNCTIONS, ref_harness.lift_functions("core/utils/skeleton_utils.py", REFERENCE_FUNCTIONS, {"np": np})))
    s = ref.scene(8, 512, 512, 11 + focal_stride + 2 * with_centers, focal_stride=focal_stride, with_centers=with_centers)
    focals = s["focals"][:, 0] if focal_stride == 1 else s["focals"]
    f64 = lambda a: None if a is None else a.astype(np.float64)      # noqa: E731
    uv32 = fn["skeleton3d_to_2d"](s["kps"], s["c2ws"], 512, 512, focals, s["centers"])
    uv64 = fn["skeleton3d_to_2d"](f64(s["kps"]), f64(s["c2ws"]), 512, 512, f64(focals), f64(s["centers"]))
    assert uv32.dtype == F32 and uv64.dtype == np.float64 and uv64.shape == (8, J, 2)
    ours = ref.host_uv(s["kps"], ref.w2c_of(s["c2ws"]), s["focals"], s["centers"], 512, 512)
    delta = float(np.abs(uv32.astype(np.float64) - uv64).max())
    dev = float(np.abs(ours.astype(np.float64) - uv64).max())
    print(f"focal_stride {focal_stride}, centers {with_centers}: delta (reference float32 against float64) = {delta:.3e} px, "
          f"this restatement against float64 = {dev:.3e} px")
    assert 0 < uv64.min() and uv64.max() < 512 and delta > 0
    assert dev <= 4 * delta
    # and the Python entry's ends are the rounded points of the same projection
    assert ref.same_bits(ref.host_project(s["kps"], ref.w2c_of(s["c2ws"]), s["focals"], s["centers"], 512, 512),
                         ref.ends_from_uv(ours[..., 0], ours[..., 1]))


# ----------------------------------------------------------------------------- properties of the rule
def _random_segments(n, seed, lo=-20, hi=80):
    return np.random.default_rng(seed).integers(lo, hi, (n, 4)).astype(np.int32)


def test_width_one_leaves_no_gap():
    for e in np.concatenate([_random_segments(60, 0), _ends((0, 0, 40, 40), (0, 0, 40, -40), (3, 5, 60, 5), (7, 2, 7, 50), (0, 0, 50, 25))]):
        ax, ay, bx, by = (int(c) for c in e)
        if abs(by - ay) <= abs(bx - ax):
            for x in range(min(ax, bx), max(ax, bx) + 1):
                assert any(c_covers(e, x, y, 1) for y in range(min(ay, by), max(ay, by) + 1)), (e, x)
        else:
            for y in range(min(ay, by), max(ay, by) + 1):
                assert any(c_covers(e, x, y, 1) for x in range(min(ax, bx), max(ax, bx) + 1)), (e, y)


def test_swapping_the_ends_changes_nothing():
    segs = np.concatenate([_random_segments(12, 1, 0, 40), ref.direct_ends()[0][[3, 7, 12, 20]]])
    for e in segs:
        swapped = e[[2, 3, 0, 1]]
        for w in (1, 2, 3, 8, 64):
            for y in range(0, 40, 1 if w < 8 else 3):
                for x in range(0, 40):
                    assert c_covers(e, x, y, w) == c_covers(swapped, x, y, w), (e, x, y, w)


def test_the_degenerate_segment_is_the_disc():
    for w in range(1, 65):
        e = _ends((40, 41, 40, 41))[0]
        r = (w + 1) // 2 + 2
        got = {(x, y) for y in range(41 - r, 42 + r) for x in range(40 - r, 41 + r) if c_covers(e, x, y, w)}
        want = {(x, y) for y in range(41 - r, 42 + r) for x in range(40 - r, 41 + r) if (x - 40) ** 2 + (y - 41) ** 2 <= (w * w) // 4}
        assert got == want and (40, 41) in got, w
    assert len({(x, y) for y in range(30, 50) for x in range(30, 50) if c_covers(_ends((40, 41, 40, 41))[0], x, y, 1)}) == 1


def test_a_later_bone_wins_where_two_cross():
    ends = np.zeros((1, J, 4), np.int32)
    ends[:, :, 0] = SKIP
    ends[0, 4] = (2, 2, 28, 28)
    ends[0, 13] = (28, 2, 2, 28)
    table = ref.colours()
    src = np.zeros((1, 31, 31, 3), np.uint8)
    for w in (1, 3):
        img = ref.host_draw(src, ends, table, w)
        assert img[0, 15, 15].tolist() == table[13].tolist() and img[0, 5, 5].tolist() == table[4].tolist()
        assert img[0, 5, 25].tolist() == table[13].tolist() and img[0, 0, 15].tolist() == [0, 0, 0]
        # the other order: the same pixels, the other colour at the crossing
        other = ends.copy()
        other[0, 4], other[0, 13] = ends[0, 13], ends[0, 4]
        img2 = ref.host_draw(src, other, table, w)
        assert np.array_equal(img2.any(-1), img.any(-1)) and img2[0, 15, 15].tolist() == table[13].tolist()
        assert img2[0, 5, 5].tolist() == table[13].tolist()


def test_ends_at_the_limits_take_the_128_bit_branch():
    """frame 0 of the direct case: every end at +-2^30, the visible part inside the 37 x 53 frame"""
    e = ref.direct_ends()[0]
    m = ref.bones_of("direct", 1)[0]
    assert set(np.unique(m).tolist()) == {-1, 3, 7, 12, 20}
    ys, xs = np.nonzero(m == 3)
    # y = x + 9: nothing beside the diagonal, and all of it but where a later bone crosses
    assert np.array_equal(ys, xs + 9) and len(xs) > 20 and all(m[x + 9, x] >= 3 for x in range(37 - 9))
    assert np.all(m[:, 26] == 20) and np.count_nonzero(m == 20) == 37           # the vertical one: its column, nothing else
    # 2 |cross| and L really are past 64-bit products here
    ax, ay, bx, by = (int(c) for c in e[7])
    L = (bx - ax) ** 2 + (by - ay) ** 2
    assert L > 2 ** 62 and (2 * abs((10 - ax) * (by - ay) - (30 - ay) * (bx - ax))) ** 2 > 2 ** 64
    # clamping: ends beyond the limits read as the limits
    beyond = _ends((-2 ** 31 + 1, -LIMIT + 9, 2 ** 31 - 1, LIMIT + 9))[0]
    assert all(c_covers(beyond, x, y, 3) == c_covers(_ends((-LIMIT, -LIMIT + 9, LIMIT, LIMIT))[0], x, y, 3) for x in range(53) for y in range(37))


# ----------------------------------------------------------------------------- quantisation of float sources
def test_quantisation_is_numpys_made_total():
    lib = ref.host_lib()
    q = lambda v: lib.ref_skel_quant(float(F32(v)))      # noqa: E731
    assert [q(0.0), q(1.0), q(0.999999), q(float("nan")), q(-0.1), q(1.5), q(-0.0), q(float("inf")), q(float("-inf"))] == [0, 255, 254, 0, 0, 255, 0, 255, 0]
    for k in range(1, 256):
        at, under = F32(k / 255), np.nextafter(F32(k / 255), F32(0))
        for v in (at, under):
            assert q(v) == int((np.array([v], F32) * 255).astype(np.uint8)[0]) == int(np.trunc(F32(v) * F32(255)))
        assert q(under) in (k - 1, k) and q(at) in (k - 1, k)
    vals = np.random.default_rng(5).random(4096, dtype=F32)
    assert [q(v) for v in vals] == (vals * 255).astype(np.uint8).tolist()
    assert ref.same_bits(ref.quantise(ref.SPECIAL), np.array([q(v) for v in ref.SPECIAL], np.uint8))


# ----------------------------------------------------------------------------- the header and its binding
def test_header_is_a_satellite_of_the_table():
    """what tests/test_abi_binding.py's referee does not hold: the host restatement is typed as the header types the entries"""
    from core import _hip
    assert "danbo_skel.h" in _hip.HEADERS
    h = _hip.header("danbo_skel.h")
    assert os.path.samefile(h.path, os.path.join(ROOT, "include", "danbo_skel.h"))
    assert h.signatures["danbo_skel_project"] == ref.PROJECT_ARGTYPES + [ctypes.c_void_p]          # + the stream
    assert h.signatures["danbo_skel_draw"] == ref.DRAW_ARGTYPES + [ctypes.c_void_p]


# ----------------------------------------------------------------------------- argument checks (no GPU: nothing is launched)
_PROJECT = ["kps", "w2c", "focals", "focal_stride", "centers", "N", "H", "W", "ends"]
_DRAW = ["src", "src_is_float", "ends", "colours", "width", "N", "H", "W", "dst"]


def _show(v):
    """an address as its offset from P: a test's name must not change with where a process happens to place a buffer"""
    return v if not isinstance(v, int) or v < P else ("P" if v == P else f"P+{v - P}")


_ids = lambda kw: "-".join(f"{k}={_show(v)}" for k, v in kw.items())      # noqa: E731


def project_call(**kw):
    a = dict(kps=P, w2c=P, focals=P, focal_stride=1, centers=None, N=1, H=4, W=4, ends=P)
    assert set(kw) <= set(a)
    a.update(kw)
    return entry("danbo_skel_project")(*(a[k] for k in _PROJECT), None)


def draw_call(**kw):
    # (dst far from src: the ranges of a 4 x 4 frame do not meet)
    a = dict(src=P, src_is_float=1, ends=P, colours=P, width=3, N=1, H=4, W=4, dst=P + 4096)
    assert set(kw) <= set(a)
    a.update(kw)
    return entry("danbo_skel_draw")(*(a[k] for k in _DRAW), None)


_DIMS = [dict(H=0), dict(H=4097), dict(W=0), dict(W=4097), dict(N=0), dict(N=-1), dict(H=-4)]


@pytest.mark.parametrize("kw", _DIMS + [dict(kps=None), dict(w2c=None), dict(focals=None), dict(ends=None), dict(focal_stride=3),
                                        dict(focal_stride=0), dict(kps=P + 2), dict(ends=P + 1), dict(centers=P + 2)], ids=_ids)
def test_project_rejects_before_any_launch(kw):
    assert project_call(**kw) == EINVAL


@pytest.mark.parametrize("kw", _DIMS + [dict(src=None), dict(ends=None), dict(colours=None), dict(dst=None), dict(width=0), dict(width=65),
                                        dict(width=-3), dict(src_is_float=2), dict(dst=P), dict(dst=P + 8), dict(src=P + 4096 + 40),
                                        dict(src_is_float=0, dst=P + 47), dict(ends=P + 2), dict(src=P + 2)], ids=_ids)
def test_draw_rejects_before_any_launch(kw):
    assert draw_call(**kw) == EINVAL


def test_restatement_rejects_the_same():
    src = np.zeros((1, 4, 4, 3), np.uint8)
    ends = np.zeros((1, J, 4), np.int32)
    assert ref.host_draw(src, ends, ref.colours(), 3, rc_only=True) == 0
    assert ref.host_draw(src, ends, ref.colours(), 0, rc_only=True) == EINVAL and ref.host_draw(src, ends, ref.colours(), 65, rc_only=True) == EINVAL
    lib = ref.host_lib()
    assert lib.ref_skel_draw(src.ctypes.data, 0, ends.ctypes.data, ref.colours().ctypes.data, 3, 1, 4, 4, src.ctypes.data) == EINVAL
    assert lib.ref_skel_project(None, None, None, 1, None, 1, 4, 4, None) == EINVAL


# ----------------------------------------------------------------------------- the Python wrappers and the flags (no GPU)
def test_wrappers_refuse_host_tensors():
    import torch
    from core.utils.skeleton_draw import draw_skeletons, draw_skeletons_3d, skeleton3d_to_2d
    img = torch.zeros(1, 4, 4, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        draw_skeletons(img, torch.zeros(1, J, 4, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        draw_skeletons_3d(img, np.zeros((1, J, 3), F32), np.eye(4, dtype=F32)[None], 4, 4, 5.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        skeleton3d_to_2d(torch.zeros(1, J, 3), np.eye(4, dtype=F32)[None], 4, 4, 5.0)


def test_render_flags_parse():
    import run_render
    base = ["--nerf_args", "a.txt", "--ckptpath", "c.tar", "--dataset", "synthetic", "--entry", "val", "--runname", "r"]
    a = run_render.config_parser().parse_args(base)
    assert a.render_skel is False and a.skel_width == 3 and a.skel_flip is False
    a = run_render.config_parser().parse_args(base + ["--render_skel", "--skel_width", "5", "--skel_flip"])
    assert a.render_skel is True and a.skel_width == 5 and a.skel_flip is True
