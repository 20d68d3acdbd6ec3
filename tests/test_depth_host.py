"""Depth and normal maps (include/danbo_depth.h), the part that needs no GPU: the serial restatement of csrc/depth_math.hpp against
the independent float64 statement of tests/depth_ref.py -- the expected depth within n 2^-24 sum|w z|, the level depth inside its
acceptance set, the normals within the bound normals64 derives (proportional to focal 2^-24) and on an exact plane --, the fixed
orders, the edge rays, the binding of the header, the argument checks (which return before any launch), the wrappers and the flags."""
import ctypes
import os

import numpy as np
import pytest

import depth_ref as ref
from helpers import ADDR as P, EINVAL, ROOT, entry        # P: an address no check follows

F32, F64, U = ref.F32, ref.F64, ref.U
LEVELS = (0.5, 1.0, 0.125)


# ----------------------------------------------------------------------------- the fixed orders
def test_the_scan_tree_is_an_inclusive_prefix():
    """on small integers every sum is exact: the tree gives the prefix sums, whatever its order"""
    x = np.random.default_rng(0).integers(0, 9, 64).astype(F32)
    assert ref.same_bits(ref.host_wave_scan(x), np.cumsum(x, dtype=F32))
    for lane in (0, 15, 16, 31, 32, 47, 63):
        e = np.zeros(64, F32)
        e[lane] = 1
        assert ref.host_wave_scan(e).tolist() == [0.0] * lane + [1.0] * (64 - lane)


def test_the_scan_tree_has_the_stated_order():
    """three values whose sum depends on the order, placed so that the tree's order is visible: 2^24 in the last lane of row 0,
    1 and 1 in the first two lanes of row 1.  Step 1 adds 1 + 1 inside row 1; row 0's total arrives in step 5: (1 + 1) + 2^24,
    exact.  A chain from lane 0 would have formed (2^24 + 1) + 1 and lost both ones."""
    big, one = F32(2.0 ** 24), F32(1.0)
    x = np.zeros(64, F32)
    x[15], x[16], x[17] = big, one, one
    s = ref.host_wave_scan(x)
    assert float(s[17]) == float(F32(F32(one + one) + big)) == 2.0 ** 24 + 2          # (1 + 1) + 2^24: exact
    assert float(F32(F32(big + one) + one)) == 2.0 ** 24                              # the chain would have lost both
    assert float(s[63]) == 2.0 ** 24 + 2


def test_lane_partial_sums_then_the_tree():
    """n = 65: position 64 is lane 0's second term -- added to position 0's before anything else"""
    w, z = np.zeros((1, 65), F32), np.ones((1, 65), F32)
    w[0, 0], w[0, 1], w[0, 64] = 2.0 ** 24, 1.0, 1.0
    d, _ = ref.host_composite(w, z, 0.5)
    assert float(d[0]) == float(F32(F32(F32(2.0 ** 24) + F32(1)) + F32(1))) == 2.0 ** 24          # (2^24 + 1) + 1, both lost
    w[0, 1], w[0, 65 - 1], w[0, 2] = 0, 0, 2.0
    d, _ = ref.host_composite(w, z, 0.5)
    assert float(d[0]) == 2.0 ** 24 + 2


# ----------------------------------------------------------------------------- per ray against float64
@pytest.mark.parametrize("n", ref.N_CASES)
def test_expected_depth_against_float64(n):
    """|depth - depth64| <= n 2^-24 sum|w z| (depth_ref's head derives it; the issue states it)"""
    c = ref.composite_case(n)
    got, _ = ref.composite_expected(n, 0.5)
    want, _ = ref.depth64(c["w"], c["z"])
    err, bound = np.abs(got.astype(F64) - want), ref.depth_bound(c["w"], c["z"])
    print(f"n = {n}: max |depth - depth64| = {err.max():.3e}, largest err / bound = {np.max(err / np.maximum(bound, 1e-300)):.3f}")
    assert np.all(err <= bound)
    assert np.all(np.isfinite(got)) and float(want.max()) > 1.0
    assert ref.same_bits(got[c["rays"]["all_zero"]], F32(0))                          # +0, not -0
    r = c["rays"]["zero_weight_nan_depth"]
    assert np.isfinite(got[r]) and (n == 1 or np.isnan(c["z"][r]).sum() == 1)
    for level in LEVELS[1:]:                                                          # the level does not touch the sum
        assert ref.same_bits(ref.composite_expected(n, level)[0], got)


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("n", ref.N_CASES)
def test_level_depth_lies_in_its_acceptance_set(n, level):
    """the returned value is z_k of a position whose float64 prefix is >= level - n 2^-24 while the prefix before it is
    < level + n 2^-24, or +0 where the total stays below level + n 2^-24 (depth_ref's head)"""
    c = ref.composite_case(n)
    _, got = ref.composite_expected(n, level)
    assert ref.level_accepts(got, c["w"], c["z"], level) == []
    total = ref.prefix64(c["w"])[:, -1]
    print(f"n = {n}, level = {level}: {int((total >= level).sum())} of {len(total)} rays reach the level")
    rays, z = c["rays"], c["z"]
    assert ref.same_bits(got[rays["all_zero"]], F32(0))
    if level == 0.5:
        assert total[rays["below_level"]] < 0.5 - n * U and ref.same_bits(got[rays["below_level"]], F32(0))
        # the prefix equals the level exactly: that position, not the next one
        want = z[rays["exact_tie"], 0 if n == 1 else ref.tie_positions(n)[1]]
        assert ref.same_bits(got[rays["exact_tie"]], want)
        if "tie_across_strips" in rays:
            assert ref.same_bits(got[rays["tie_across_strips"]], z[rays["tie_across_strips"], 64])
        # (the case holds rays on both sides of the level; a single position rarely carries half the weight)
        assert int((total >= 0.5 + n * U).sum()) >= (5 if n == 1 else 20) and int((total < 0.5 - n * U).sum()) >= 2
    if level == 1.0:
        assert total[rays["exact_one"]] == 1.0 and ref.same_bits(got[rays["exact_one"]], z[rays["exact_one"], n - 1])
        assert ref.same_bits(got[rays["exact_tie"]], F32(0)) and ref.same_bits(got[rays["below_level"]], F32(0))
    # a reached level names a depth of the ray: ascending depths, so a higher level is never nearer
    lo = ref.composite_expected(n, 0.125)[1]
    assert np.all((got == 0) | (got >= lo) | np.isnan(got))


@pytest.mark.parametrize("n", (18, 65))
def test_restatement_walks_the_ray_list(n):
    c = ref.ray_list_case(n)
    d, l = ref.host_composite(c["w"], c["z"], 0.5, c["ray_list"], c["ray_count"], init=ref.SENTINEL)
    full_d, full_l = ref.composite_expected(n, 0.5)
    listed = c["listed"]
    assert int(listed.sum()) == 41
    assert ref.same_bits(d[listed], full_d[listed]) and ref.same_bits(l[listed], full_l[listed])
    assert np.all(d[~listed] == ref.SENTINEL) and np.all(l[~listed] == ref.SENTINEL)
    # a count beyond R reads as R, a negative one as 0; an entry outside 0 .. R - 1 is clamped
    none = ref.host_composite(c["w"], c["z"], 0.5, c["ray_list"], -3, init=ref.SENTINEL)
    assert np.all(none[0] == ref.SENTINEL) and np.all(none[1] == ref.SENTINEL)
    w, z = ref.composite_case(n)["w"], ref.composite_case(n)["z"]
    clamp = ref.host_composite(w, z, 0.5, np.array([-9, 10 ** 6] + [0] * (ref.R_RAYS - 2), np.int32), 2, init=ref.SENTINEL)
    assert ref.same_bits(clamp[0][[0, -1]], full_d[[0, -1]]) and np.all(clamp[0][1:-1] == ref.SENTINEL)


# ----------------------------------------------------------------------------- per pixel against float64
@pytest.mark.parametrize("kw", ref.NORMAL_VARIANTS, ids=lambda kw: f"jump={kw['jump']}-space={kw['space']}")
def test_normals_against_float64(kw):
    """every colour channel within normals64's per-pixel bound (2 e_c / |c| + 14 u, ~ 32 u focal: the cancellation in the
    differences) of the float64 evaluation of the same formulas on the same fp32 inputs; the same pixels have a normal"""
    c = ref.frames_case()
    rgb, valid = ref.normals_expected(kw["jump"], kw["space"])
    want, ok, bound = ref.normals64(c["depth"], c["acc"], c["cast"], c["c2w"], c["intr"], 0.5, kw["jump"], kw["space"], 1.0)
    assert np.array_equal(valid.astype(bool), ok) and set(np.unique(valid).tolist()) == {0, 1}
    err = np.abs(rgb.astype(F64) - want).max(-1)
    focal = float(c["intr"][:, :2].max())
    print(f"{kw}: {int(ok.sum())} of {ok.size} pixels with a normal; max err {err.max():.3e}, max bound {bound.max():.3e} "
          f"(= {bound.max() / (focal * U):.1f} focal u), largest err / bound {np.max(err[ok] / bound[ok]):.3f}")
    assert np.all(err <= bound)
    assert bound.max() < 256 * focal * U                                  # the bound itself is of the order of focal 2^-24
    assert np.all(rgb[valid == 0] == 1.0)                                 # the background, exactly
    n = 2 * rgb[valid == 1].astype(F64) - 1
    assert np.abs(np.linalg.norm(n, axis=-1) - 1).max() < 1e-5
    if kw["space"] == 0:
        assert np.all(n[:, 2] > 0)                                        # towards the camera


def test_holes_borders_and_the_jump():
    c = ref.frames_case()
    off, on = ref.normals_expected(0.0, 0)[1].astype(bool), ref.normals_expected(0.4, 0)[1].astype(bool)
    acc, cast = c["acc"], c["cast"]
    # unusable pixels have no normal: not cast, transparent, below the threshold; at the threshold exactly: usable
    assert not off[cast == 0].any() and not off[acc < 0.5].any() and off[0, 8, 4] and acc[0, 8, 4] == 0.5
    assert not off[0, 7, 1] and acc[0, 7, 1] >= 0.5 and cast[0, 7, 1]        # usable, but nothing usable above or below it
    assert not off[1, 6, 8] and acc[1, 6, 8] >= 0.5                          # usable, but nothing usable left or right of it
    assert off[0, 0, 1] and off[0, 8, 10] and off[1, 0, 0] and off[1, 8, 0]  # border and corner pixels: one-sided differences
    assert off[0, 4, 4] and off[0, 4, 6] and off[0, 3, 5]                    # beside a hole: one-sided too
    # the jump only ever removes neighbours; along the step of frame 1 a pixel with a usable neighbour on its own side keeps a
    # normal, and the normal changes: it no longer averages across the step
    assert not (on & ~off).any()
    a, b = ref.normals_expected(0.0, 0)[0], ref.normals_expected(0.4, 0)[0]
    changed = np.abs(a - b).max(-1) > 1e-3
    assert on[1][1:5, 5:7].all() and off[1, 6, 6] and not on[1, 6, 6]      # (6, 6): the step on one side, a hole on the other
    assert changed[1][1:5, 5:7].all() and not changed[1][:, :4].any() and not changed[0].any()      # (rows 1 .. 4: no hole nearby)
    # without the cast mask the pixels that were not cast have acc 0: the same map
    assert ref.same_bits(ref.normals_expected(0.0, 0, with_cast=False)[0], a)


@pytest.mark.parametrize("space", [0, 1])
def test_exact_plane(space):
    """A tilted plane at 9 x 11 pixels.  The float64 formulas on the exact depths give the plane's normal (the differences of points
    of a plane lie in it) to float64 round-off; the fp32 restatement on the depths rounded to fp32 is within twice its bound of
    it -- the rounding of the input is one more relative 2^-24 on D, where the bound already allows four and is doubled."""
    c2w, intr = ref.cameras(2)
    D = ref.plane_depth(intr)
    ones = np.ones_like(D)
    want = ref.PLANE_NORMAL if space == 0 else np.einsum("nij,j->ni", c2w[:, :, :3].astype(F64), ref.PLANE_NORMAL)[:, None, None, :]
    rgb64, ok, _ = ref.normals64(D, ones, None, c2w, intr, 0.5, 0.0, space, 1.0)
    assert ok.all() and np.abs(2 * rgb64 - 1 - want).max() < 1e-12
    rgb, valid = ref.host_normals(D.astype(F32), ones.astype(F32), None, c2w, intr, 0.5, 0.0, space, 1.0)
    _, _, bound = ref.normals64(D.astype(F32), ones, None, c2w, intr, 0.5, 0.0, space, 1.0)
    err = np.abs(rgb.astype(F64) - (0.5 * want + 0.5)).max(-1)
    print(f"plane, space {space}: fp32 against the plane's normal: max err {err.max():.3e}, largest err / (2 bound) {np.max(err / (2 * bound)):.3f}")
    assert valid.all() and np.all(err <= 2 * bound)


# ----------------------------------------------------------------------------- the header and its binding
def test_header_is_a_satellite_of_the_table():
    """what tests/test_abi_binding.py's referee does not hold: the host restatement is typed as the header types the entries"""
    from core import _hip
    assert "danbo_depth.h" in _hip.HEADERS
    h = _hip.header("danbo_depth.h")
    assert os.path.samefile(h.path, os.path.join(ROOT, "include", "danbo_depth.h"))
    assert h.signatures["danbo_depth_composite_fwd"] == ref.COMPOSITE_ARGTYPES + [ctypes.c_void_p]          # + the stream
    assert h.signatures["danbo_depth_normals"] == ref.NORMALS_ARGTYPES + [ctypes.c_void_p]


# ----------------------------------------------------------------------------- argument checks (no GPU: nothing is launched)
def composite_args(**kw):
    return ref.composite_args(P, **kw)


def normals_args(**kw):
    return ref.normals_args(P, **kw)


COMPOSITE_REJECTS, NORMALS_REJECTS, _ids = ref.COMPOSITE_REJECTS, ref.NORMALS_REJECTS, ref.reject_id


@pytest.mark.parametrize("kw", COMPOSITE_REJECTS, ids=_ids)
def test_composite_rejects_before_any_launch(kw):
    assert entry("danbo_depth_composite_fwd")(*composite_args(**kw), None) == EINVAL
    assert ref.host_lib().ref_depth_composite(*composite_args(**kw)) == EINVAL          # the restatement rejects the same


@pytest.mark.parametrize("kw", NORMALS_REJECTS, ids=_ids)
def test_normals_rejects_before_any_launch(kw):
    assert entry("danbo_depth_normals")(*normals_args(**kw), None) == EINVAL
    assert ref.host_lib().ref_depth_normals(*normals_args(**kw)) == EINVAL


def test_empty_batch_is_accepted_without_a_launch():
    assert entry("danbo_depth_composite_fwd")(*composite_args(R=0), None) == 0


# ----------------------------------------------------------------------------- the Python wrappers and the flags (no GPU)
def test_wrappers_refuse_host_tensors():
    import torch
    from core.depth_maps import composite_depth, normal_maps
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        composite_depth(torch.zeros(3, 18), torch.zeros(3, 18))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        normal_maps(torch.zeros(1, 4, 4), torch.zeros(1, 4, 4), np.eye(4, dtype=F32)[None], 5.0)


def test_camera_rows():
    from core.depth_maps import camera_rows
    c2w = np.arange(32, dtype=F32).reshape(2, 4, 4)
    rows, intr = camera_rows(c2w, 7.5, None, 2, 9, 11, "cpu")
    assert rows.shape == (2, 3, 4) and np.array_equal(rows.numpy(), c2w[:, :3]) and intr.tolist() == [[7.5, 7.5, 5.5, 4.5]] * 2
    _, intr = camera_rows(c2w[:, :3], np.array([[7.0, 8.0], [9.0, 10.0]]), np.array([[1.0, 2.0], [3.0, 4.0]]), 2, 9, 11, "cpu")
    assert intr.tolist() == [[7.0, 8.0, 1.0, 2.0], [9.0, 10.0, 3.0, 4.0]]
    _, intr = camera_rows(c2w, np.array([7.0, 9.0]), None, 2, 9, 11, "cpu")
    assert intr[:, :2].tolist() == [[7.0, 7.0], [9.0, 9.0]]
    with pytest.raises(ValueError):
        camera_rows(c2w, np.zeros((2, 3)), None, 2, 9, 11, "cpu")


def test_render_flags_parse():
    import run_render
    base = ["--nerf_args", "a.txt", "--ckptpath", "c.tar", "--dataset", "synthetic", "--entry", "val", "--runname", "r"]
    a = run_render.config_parser().parse_args(base)
    assert a.render_depth is False and a.depth_level == 0.5 and a.render_normal is False and a.normal_space == "camera"
    assert a.normal_acc_min == 0.5 and a.normal_jump == 0.0
    a = run_render.config_parser().parse_args(base + ["--render_depth", "--depth_level", "0.9", "--render_normal", "--normal_space", "world",
                                                      "--normal_acc_min", "0.25", "--normal_jump", "0.05"])
    assert a.render_depth and a.depth_level == 0.9 and a.render_normal and a.normal_space == "world"
    assert a.normal_acc_min == 0.25 and a.normal_jump == 0.05
    with pytest.raises(SystemExit):
        run_render.config_parser().parse_args(base + ["--normal_space", "object"])


def test_render_path_and_engines_take_the_arguments():
    import inspect
    import run_nerf
    from core.anerf_engine import AnerfEngine
    from core.raycasters import RayCaster
    from core.render_engine import DanboEngine
    assert inspect.signature(run_nerf.render_path).parameters["ret_depth"].default is False
    for fn in (DanboEngine.render, DanboEngine.render_two_net, AnerfEngine.render):
        p = inspect.signature(fn).parameters
        assert p["depth"].default is False and p["depth_level"].default == 0.5
    for fn in (RayCaster.render_rays, RayCaster.render_rays_whole):
        p = inspect.signature(fn).parameters
        assert p["render_depth"].default is False and p["depth_level"].default == 0.5
    assert RayCaster._depth_kwargs(False, 0.5) == {} and RayCaster._depth_kwargs(True, 0.25) == dict(depth=True, depth_level=0.25)
