"""Connected components of a density grid and the floater filter (include/danbo_grid_cc.h), the part that needs no GPU: the serial
restatement of csrc/grid_cc_math.hpp against scipy.ndimage.label bit for bit, the keep rule, the two properties the header states
(vertices survive unchanged; the layout does not matter), the binding of the header and the argument checks, which return before
any launch.  Every comparison is exact."""
import ctypes
import os

import numpy as np
import pytest

import grid_cc_ref as ref
import mesh_ref
from helpers import ADDR as P, EINVAL, ROOT, entry        # P: an address no check follows

F32 = np.float32
INF = float("inf")
# the counts of the grids whose content is fixed: name -> (components, sizes in descending order or None, label of the largest)
KNOWN = {"two_spheres": (2, [557, 313], None), "noise0": (202, None, None), "noise1": (219, None, None),
         "serpentine": (3, [339, 339, 339], 0), "snake": (1, [1699], 0)}
LARGEST = {"noise0": 8446, "noise1": 8461}


# ----------------------------------------------------------------------------- the restatement against scipy
@pytest.mark.parametrize("name", sorted(ref.cases()))
def test_restatement_equals_scipy(name):
    sigma, iso, floor = ref.cases()[name]
    labels, sizes, stats = ref.reference(name)
    want = ref.predict(sigma, iso, floor)
    assert ref.same_bits(labels, want[0]) and ref.same_bits(sizes, want[1]) and ref.same_bits(stats, want[2]), (stats, want[2])
    # the definitions, read back: a label is the first index of its component, sizes sit at labels only and add up to the inside set
    lin = np.arange(sigma.size).reshape(sigma.shape)
    inside = ref.inside_set(sigma, iso, floor)
    assert np.array_equal(labels >= 0, inside) and np.all(labels[inside] <= lin[inside])
    assert sizes.sum() == stats[0] == inside.sum() and np.count_nonzero(sizes) == stats[1]
    assert np.array_equal(np.flatnonzero(sizes), np.unique(labels[inside]))
    without = ref.host_label(sigma, iso, floor, want_sizes=False)
    assert without[1] is None and ref.same_bits(without[0], labels) and ref.same_bits(without[2], stats)


@pytest.mark.parametrize("name", sorted(KNOWN))
def test_the_counts_of_the_fixed_grids(name):
    n, sizes_desc, label = KNOWN[name]
    _, sizes, stats = ref.reference(name)
    assert stats[1] == n
    if sizes_desc is not None:
        assert sorted(sizes[sizes > 0].tolist(), reverse=True) == sizes_desc and stats[2] == sizes_desc[0]
    if label is not None:
        assert stats[3] == label
    if name in LARGEST:
        assert stats[2] == LARGEST[name] and np.count_nonzero(sizes == LARGEST[name]) == 1
    if name == "serpentine":
        assert np.flatnonzero(sizes).tolist() == [0, 1206, 2412]


def test_small_grids_have_the_obvious_answers():
    for shape in ref.SMALL_SHAPES:
        n = int(np.prod(shape))
        tag = "_%dx%dx%d" % shape
        assert ref.reference("all_inside" + tag)[2].tolist() == [n, 1, n, 0]
        assert ref.reference("all_outside" + tag)[2].tolist() == [0, 0, 0, -1]
        one = np.ravel_multi_index(tuple(s // 2 for s in shape), shape)
        assert ref.reference("one_point" + tag)[2].tolist() == [1, 1, 1, one]
        sigma = ref.cases()["nan_inf" + tag][0]
        labels = ref.reference("nan_inf" + tag)[0]
        assert np.all(labels[np.isnan(sigma) | (sigma == -INF)] == -1) and np.all(labels[sigma == INF] >= 0)


def test_bernoulli_grids_are_the_three_regimes():
    comps = [int(ref.reference(f"bernoulli_{p}")[2][1]) for p in ref.BERNOULLI_P]
    big = [int(ref.reference(f"bernoulli_{p}")[2][2]) for p in ref.BERNOULLI_P]
    assert 1.8e4 < comps[0] < 2.2e4 and big[0] < 200                  # many small components
    assert 2.2e3 < comps[2] < 3.2e3 and big[2] > 0.45 * 64 ** 3       # one giant component and the rest
    assert big[0] < big[1] < big[2]


# ----------------------------------------------------------------------------- the keep rule
@pytest.mark.parametrize("keep_largest, min_points, labels_kept",
                         [(True, 0, [0]), (False, 339, [0, 1206, 2412]), (False, 340, []), (True, 339, [0]), (True, 340, []),
                          (False, 0, [0, 1206, 2412])])
def test_keep_rule_on_the_serpentine(keep_largest, min_points, labels_kept):
    sigma, iso, floor = ref.cases()["serpentine"]
    labels, sizes, stats = ref.reference("serpentine")
    out, kept = ref.host_keep(sigma, iso, floor, labels, sizes, stats, keep_largest, min_points)
    assert kept.tolist() == [len(labels_kept), 339 * len(labels_kept)]
    want = sigma.copy()
    want[(labels >= 0) & ~np.isin(labels, labels_kept)] = -INF
    assert ref.same_bits(out, want)
    assert sorted(np.unique(ref.host_label(out, iso, floor)[0]).tolist()) == sorted([-1] + labels_kept)


@pytest.mark.parametrize("name", ["two_spheres", "noise0", "bernoulli_0.3116", "nan_inf_3x5x65", "floor0_iso10_2x3x1024", "all_outside_2x2x2"])
def test_keep_equals_the_numpy_rule(name):
    sigma, iso, floor = ref.cases()[name]
    labels, sizes, stats = ref.reference(name)
    for keep_largest, min_points in ((False, 0), (True, 0), (False, 5), (True, 10 ** 6)):
        fill = ref.default_fill(iso, floor)
        for transposed_out in (False, True):
            out, kept = ref.host_keep(sigma, iso, floor, labels, sizes, stats, keep_largest, min_points, transposed_out=transposed_out)
            want, want_kept = ref.predict_keep(sigma, labels, sizes, stats, keep_largest, min_points, fill)
            assert ref.same_bits(out, want) and ref.same_bits(kept, want_kept)          # (by bytes: the NaNs are kept)
        if not keep_largest and not min_points:
            assert ref.same_bits(out, np.ascontiguousarray(sigma))


def test_keep_in_place_gives_the_same_grid():
    sigma, iso, floor = ref.cases()["noise1"]
    labels, sizes, stats = ref.reference("noise1")
    want, want_kept = ref.host_keep(sigma, iso, floor, labels, sizes, stats, True, 0)
    buf, view = mesh_ref.guarded(sigma.size, F32)
    work = view.reshape(sigma.shape)
    work[:] = sigma
    kept = np.zeros(2, np.int32)
    a = [np.ascontiguousarray(x, np.int32) for x in (labels, sizes, stats)]
    rc = ref.host_lib().ref_grid_keep(*ref.grid_args(work, iso, floor), *(x.ctypes.data for x in a), 1, 0, -INF, work.ctypes.data,
                                      work.strides[0] // 4, work.strides[1] // 4, kept.ctypes.data)
    assert rc == 0 and mesh_ref.guards_intact(buf) and ref.same_bits(work, want) and ref.same_bits(kept, want_kept)


def test_keep_rejects_what_the_header_says():
    sigma, iso, floor = ref.cases()["two_spheres"]
    labels, sizes, stats = ref.reference("two_spheres")
    keep = lambda **kw: ref.host_keep(sigma, iso, floor, labels, sizes, stats, rc_only=True, **kw)      # noqa: E731
    assert keep() == 0
    assert keep(min_points=-1) == EINVAL and keep(fill=0.) == EINVAL and keep(fill=1.) == EINVAL and keep(fill=INF) == EINVAL
    assert keep(fill=-1e-30) == 0 and keep(fill=float("nan")) == 0
    # floor = 0, iso = 10: the floor lifts every fill to 0, which is outside
    s2, iso2, floor2 = ref.cases()["floor0_iso10_3x5x65"]
    l2 = ref.reference("floor0_iso10_3x5x65")
    assert ref.host_keep(s2, iso2, floor2, *l2, fill=-5., rc_only=True) == 0
    assert ref.host_keep(s2, iso2, floor2, *l2, fill=10., rc_only=True) == EINVAL
    # out overlapping sigma without being sigma; an out whose rows share addresses
    flat = np.zeros(2 * sigma.size, F32)
    src = flat[:sigma.size].reshape(sigma.shape)
    lib, a = ref.host_lib(), [np.ascontiguousarray(x, np.int32) for x in (labels, sizes, stats)]
    call = lambda out_ptr, osx, osy: lib.ref_grid_keep(*ref.grid_args(src, iso, floor), *(x.ctypes.data for x in a), 0, 0, -INF,      # noqa: E731
                                                       out_ptr, osx, osy, None)
    nx, ny, nz = sigma.shape
    assert call(src.ctypes.data, ny * nz, nz) == 0                                  # in place
    assert call(src.ctypes.data + 4 * sigma.size, ny * nz, nz) == 0                 # right behind
    assert call(src.ctypes.data + 4, ny * nz, nz) == EINVAL                         # shifted by one element
    assert call(src.ctypes.data, nz, nx * nz) == EINVAL                             # the same memory in another layout
    assert call(src.ctypes.data + 4 * sigma.size, ny * nz, nz - 1) == EINVAL        # rows that overlap
    assert call(src.ctypes.data + 4 * sigma.size, 0, nz) == EINVAL


# ----------------------------------------------------------------------------- the two properties
def test_keep_largest_of_two_spheres_is_the_single_sphere_mesh():
    sigma, iso, floor = ref.cases()["two_spheres"]
    out, kept, stats = ref.filtered(sigma, iso, floor, keep_largest=True)
    assert stats.tolist()[:3] == [870, 2, 557] and kept.tolist() == [1, 557]
    single = (5.1 - np.linalg.norm(mesh_ref.lattice(sigma.shape) - np.array([19.2, 18.6, 19.4]), axis=-1)).astype(F32)
    v, f = mesh_ref.host_extract(out, iso)
    v1, f1 = mesh_ref.host_extract(single, iso)
    assert len(v) > 0 and ref.same_bits(v, v1) and ref.same_bits(f, f1)
    # every vertex of the filtered mesh is, bit for bit, a vertex of the unfiltered one
    v0, _ = mesh_ref.host_extract(np.ascontiguousarray(sigma), iso)
    rows = {r.tobytes() for r in v0}
    assert len(v0) > len(v) and all(r.tobytes() in rows for r in v)


@pytest.mark.parametrize("name", ["noise0", "snake", "nan_inf_3x5x65"])
def test_the_layout_does_not_matter(name):
    sigma, iso, floor = ref.cases()[name]
    swapped = np.ascontiguousarray(sigma.transpose(1, 0, 2)).transpose(1, 0, 2)       # the same logical grid, x-y transposed memory
    assert swapped.strides != sigma.strides and ref.same_bits(np.ascontiguousarray(swapped), np.ascontiguousarray(sigma))
    got = ref.host_label(swapped, iso, floor)
    assert all(ref.same_bits(a, b) for a, b in zip(got, ref.reference(name)))
    out, kept = ref.host_keep(swapped, iso, floor, *got, keep_largest=True)
    want = ref.host_keep(sigma, iso, floor, *got, keep_largest=True)
    assert ref.same_bits(out, want[0]) and ref.same_bits(kept, want[1])


# ----------------------------------------------------------------------------- the header and its binding
def test_header_is_a_satellite_of_the_table():
    """what tests/test_abi_binding.py's referee does not hold: the host restatement is typed as the header types the entries"""
    from core import _hip
    assert "danbo_grid_cc.h" in _hip.HEADERS
    h = _hip.header("danbo_grid_cc.h")
    assert os.path.samefile(h.path, os.path.join(ROOT, "include", "danbo_grid_cc.h"))
    assert h.signatures["danbo_grid_cc_label"] == ref.LABEL_ARGTYPES + [ctypes.c_void_p] * 2          # + the workspace and the stream
    assert h.signatures["danbo_grid_cc_keep"] == ref.KEEP_ARGTYPES + [ctypes.c_void_p]
    assert h.restypes["danbo_grid_cc_workspace_bytes"] is ctypes.c_size_t and h.restypes["danbo_grid_cc_label"] is ctypes.c_int


def test_workspace_bytes_has_the_limits_of_the_mesh_workspace():
    from core import _hip
    ws = entry("danbo_grid_cc_workspace_bytes")
    for dims in ((2, 2, 2), (28, 28, 28), (256, 256, 256), (1024, 1024, 1024), (2, 1024, 1024)):
        assert ws(*dims) >= 4 * int(np.prod(dims)) and _hip.lib().danbo_mesh_workspace_bytes(*dims) > 0
    for dims in ((1, 8, 8), (8, 1, 8), (8, 8, 1), (0, 8, 8), (-4, 8, 8), (1025, 8, 8), (8, 8, 1025), (2048, 1024, 1024)):
        assert ws(*dims) == 0 == _hip.lib().danbo_mesh_workspace_bytes(*dims)


# ----------------------------------------------------------------------------- argument checks (no GPU: nothing is launched)
_LABEL = ["sigma", "nx", "ny", "nz", "sx", "sy", "floor", "iso", "workspace", "labels", "sizes", "stats"]
_KEEP = ["sigma", "nx", "ny", "nz", "sx", "sy", "floor", "iso", "labels", "sizes", "stats", "keep_largest", "min_points", "fill", "out",
         "osx", "osy", "kept"]
_N = 8 * 8 * 8
REJECTED_GRIDS = [dict(sigma=None), dict(sigma=P + 2), dict(nx=1), dict(ny=1), dict(nz=1), dict(nx=1025), dict(nz=0), dict(ny=-8),
                  dict(nx=2048, ny=1024, nz=1024), dict(sx=-64), dict(sy=-8), dict(iso=INF), dict(iso=float("nan")), dict(floor=INF),
                  dict(floor=float("nan")), dict(labels=None), dict(labels=P + 1), dict(sizes=P + 2), dict(stats=None), dict(stats=P + 2)]
def _show(v):
    """an address as its offset from P: a test's name must not change with where a process happens to place a buffer"""
    return v if not isinstance(v, int) or v < P else ("P" if v == P else f"P+{v - P}")


_ids = lambda kw: "-".join(f"{k}={_show(v)}" for k, v in kw.items())      # noqa: E731


def label_call(**kw):
    a = dict(sigma=P, nx=8, ny=8, nz=8, sx=64, sy=8, floor=0., iso=10., workspace=P, labels=P, sizes=P, stats=P)
    assert set(kw) <= set(a)
    a.update(kw)
    return entry("danbo_grid_cc_label")(*(a[k] for k in _LABEL), None)


def keep_call(**kw):
    # (out far from sigma: the two ranges of an 8^3 grid do not meet)
    a = dict(sigma=P, nx=8, ny=8, nz=8, sx=64, sy=8, floor=0., iso=10., labels=P, sizes=P, stats=P, keep_largest=1, min_points=0, fill=0.,
             out=P + 4 * _N, osx=64, osy=8, kept=P)
    assert set(kw) <= set(a)
    a.update(kw)
    return entry("danbo_grid_cc_keep")(*(a[k] for k in _KEEP), None)


@pytest.mark.parametrize("kw", REJECTED_GRIDS + [dict(workspace=None), dict(workspace=P + 4)], ids=_ids)
def test_label_rejects_before_any_launch(kw):
    assert label_call(**kw) == EINVAL


@pytest.mark.parametrize("kw", REJECTED_GRIDS + [dict(sizes=None), dict(out=None), dict(out=P + 4 * _N + 2), dict(kept=P + 2), dict(min_points=-1),
                                                 dict(fill=10.), dict(fill=INF), dict(floor=-INF, fill=10.), dict(out=P + 4), dict(out=P, osx=8, osy=64),
                                                 dict(osy=7), dict(osx=63), dict(osx=0), dict(osx=-64)], ids=_ids)
def test_keep_rejects_before_any_launch(kw):
    assert keep_call(**kw) == EINVAL


# ----------------------------------------------------------------------------- the Python wrappers and the flags (no GPU)
def test_wrappers_refuse_host_tensors_and_bad_arguments():
    import torch
    from core.grid_components import grid_components, keep_components
    g = torch.zeros(4, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        grid_components(g, 0.)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        keep_components(g, 0., -INF, g.int(), g.int(), torch.zeros(4, dtype=torch.int32))


def test_render_flags_parse():
    import run_render
    base = ["--nerf_args", "a.txt", "--ckptpath", "c.tar", "--dataset", "synthetic", "--entry", "val", "--runname", "r", "--render_mesh"]
    a = run_render.config_parser().parse_args(base)
    assert a.mesh_keep_largest is False and a.mesh_min_points == 0
    a = run_render.config_parser().parse_args(base + ["--mesh_keep_largest", "--mesh_min_points", "64"])
    assert a.mesh_keep_largest is True and a.mesh_min_points == 64
