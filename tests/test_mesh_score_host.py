"""Mesh scores without a GPU: the serial restatement of csrc/mesh_score_math.hpp (the code the kernels inline, built by g++) against
the float64 statement of tests/mesh_score_ref.py, known answers, the argument rules, and the binding of include/danbo_mesh_score.h
as a satellite beside the headers of _hip.HEADERS.  The bounds are derived in mesh_score_ref's docstring."""
import ctypes

import numpy as np
import pytest

import mesh_score_ref as ms
from helpers import ADDR, EINVAL, entry
from mesh_score_ref import F32, F64, U

ENTRIES = ("danbo_mesh_face_areas", "danbo_mesh_sample", "danbo_points_nearest_workspace_bytes", "danbo_points_nearest", "danbo_points_score")


# ----------------------------------------------------------------------------- nearest point
@pytest.mark.parametrize("Nq, Nr", [(65, 1), (63, 1025), (1000, 3079)])
def test_nearest_restatement_against_float64(Nq, Nr):
    c = ms.nearest_case(Nq, Nr)
    bad, rel, exc = ms.nearest_rejects(c["d2"], c["idx"], c["q"], c["r"])
    print(f"nearest {Nq} x {Nr}: |d2_32 - d2_64| / d2_64 max {rel / U:.3f} u; chosen over minimum max {exc / U:.3f} u (bound 3 u)")
    assert not bad, bad[:10]


def test_nearest_with_duplicates_picks_the_lower_index():
    c = ms.nearest_case(65, 1025, "duplicates")
    bad, _, _ = ms.nearest_rejects(c["d2"], c["idx"], c["q"], c["r"])
    assert not bad
    # every chosen index is the first row of r that equals the chosen row
    r, tied = c["r"], 0
    for i, j in enumerate(c["idx"]):
        same = np.flatnonzero((r == r[j]).all(1))
        assert same[0] == j, (i, j, same)
        tied += len(same) > 1
    assert tied >= 10                               # the case does hold queries whose nearest point exists twice
    # and a reference set that is one point many times: index 0, whatever the query
    q = np.random.default_rng(1).uniform(-2, 2, (9, 3)).astype(F32)
    d2, idx = ms.host_nearest(q, np.tile(F32([[0.5, -1.25, 0.75]]), (40, 1)))
    assert np.all(idx == 0) and np.all(d2 > 0)


def test_identical_sets_and_the_shifted_cube():
    c = ms.nearest_case(1000, 1000, "self")
    assert np.all(c["d2"] == 0) and not np.signbit(c["d2"]).any()
    first = np.array([np.flatnonzero((c["r"] == p).all(1))[0] for p in c["q"]])
    assert np.array_equal(c["idx"], first) and np.array_equal(first, np.arange(1000))       # (random rows: no accidental copies)
    n = (c["q"] / np.linalg.norm(c["q"], axis=1, keepdims=True)).astype(F32)
    tau = np.array([0.01, 0.0], F32)
    out = ms.host_score(c["d2"], c["idx"], n, n, tau)
    s = ms.metrics64(out, out, (0.01, 0.0))
    assert s["chamfer_l1"] == 0 and s["chamfer_l2"] == 0 and s["fscore"] == {0.01: 1.0, 0.0: 1.0}
    assert abs(s["normal_consistency"] - 1) <= 4 * U       # |n . n| of fp32 unit vectors
    cube = np.array([(x, y, z) for x in (0, 1) for y in (0, 1) for z in (0, 1)], F32)
    d2, idx = ms.host_nearest(cube, cube + F32([0.25, 0, 0]))
    assert ms.same_bits(d2, np.full(8, 0.0625, F32)) and np.array_equal(idx, np.arange(8))
    d2, idx = ms.host_nearest(cube + F32([0.25, 0, 0]), cube)
    assert ms.same_bits(d2, np.full(8, 0.0625, F32)) and np.array_equal(idx, np.arange(8))


def test_the_key_orders_like_the_pair():
    key = ms.host_lib().ref_key
    assert key(0.0, 5) < key(0.0, 6) < key(1e-45, 0) < key(1.0, 0) < key(1.0, 1 << 24) < key(float("inf"), 0) < 2 ** 64 - 1
    assert key(0.0625, 3) == (int(np.float32(0.0625).view(np.uint32)) << 32) | 3


def test_two_icospheres():
    (va, _), (vb, fb) = ms.icosphere(2, 1.0), ms.icosphere(2, 1.1)
    va64, vb64 = va.astype(F64), vb.astype(F64)
    for q, r, r_faces in ((va, vb, fb), (vb, va, ms.icosphere(2, 1.0)[1])):
        # the two facts on the float64 statement first: vertices lie on their spheres, so no distance is below the gap between
        # the radii (taken from the fp32 vertices' own lengths), and the mean is at most the gap + 2 x the longest edge
        gap = abs(np.linalg.norm(vb64, axis=1).min() - np.linalg.norm(va64, axis=1).max())
        assert abs(gap - 0.1) < 1e-6
        dmin64 = np.sqrt(ms.nearest64(q, r)[0])
        edge = ms.longest_edge(r, r_faces)
        assert dmin64.min() >= gap * (1 - 1e-12) and dmin64.mean() <= 0.1 + 2 * edge
        d2, idx = ms.host_nearest(q, r)
        assert not ms.nearest_rejects(d2, idx, q, r)[0]
        d = np.sqrt(d2.astype(F64))
        assert d.min() >= gap * (1 - 2 * U) and d.mean() <= (0.1 + 2 * edge) * (1 + 2 * U)      # sqrt of (1 +- 3 u): 1.5 u
        out = ms.host_score(d2, idx, None, None, np.array([0.05, 0.5], F32))
        assert out[4] == 0 and out[5] == len(q) and out[3] == len(q) and out[2] == 0


# ----------------------------------------------------------------------------- sampling
def test_face_areas_against_float64():
    for name in ms.MESHES:
        verts, faces = ms.MESHES[name]()
        areas, flag = ms.host_areas(verts, faces)
        a64 = ms.areas64(verts, faces)
        v = np.abs(verts.astype(F64)[faces])
        # s = the largest |coordinate| of the face: an edge (<= 2 s) carries 2 u s, a product of two edges 12 u s^2 with its own
        # rounding, their difference 32 u s^2, the vector of three sqrt(3) x that, halved: 28 u s^2; the three roundings under the
        # root, the root and the half add < 4 u area <= 4 u 2 sqrt(3) s^2: 42 u s^2 in all
        scale = v.max((1, 2))
        assert flag == 0 and np.all(np.abs(areas - a64) <= 42 * U * scale * scale)
    verts, faces = ms.degenerate_mesh()
    areas, _ = ms.host_areas(verts, faces)
    zero = [0, 3, 5, 9]
    assert np.all(areas[zero] == 0) and np.all(np.delete(areas, zero) > 0) and areas[1] == areas[2] and areas[4] == areas[7]


@pytest.mark.parametrize("name", sorted(ms.MESHES))
def test_regular_grid_counts_per_face(name):
    """with u0 a regular grid, every face gets exactly the grid values inside its cdf interval; faces of area zero get none"""
    c = ms.sample_case(name, 1)
    M = 4096
    u = np.zeros((M, 3), F32)
    u[:, 0] = (np.arange(M, dtype=F64) / M).astype(F32)
    u[:, 1:] = np.random.default_rng(5).random((M, 2), dtype=F32)
    face = ms.host_sample(c["verts"], c["faces"], c["cdf"], u)[2]
    cdf = c["cdf"]
    target = (u[:, 0] * cdf[-1]).astype(F32)
    lower = np.concatenate([[F32(-1)], cdf[:-1]])
    expected = np.array([np.count_nonzero((target >= lower[f]) & (target < cdf[f])) for f in range(len(cdf))])
    got = np.bincount(face, minlength=len(cdf))
    assert target.max() < cdf[-1] and np.array_equal(got, expected) and np.array_equal(face, ms.pick64(cdf, u[:, 0]))
    assert np.all(got[c["areas"] == 0] == 0) and got.sum() == M
    if name == "icosphere":
        assert got.min() >= 1


@pytest.mark.parametrize("name", sorted(ms.MESHES))
def test_samples_against_float64(name):
    c = ms.sample_case(name, 1000)
    b = ms.host_bary(c["u"])
    assert np.all(b >= 0) and np.abs(b.astype(F64).sum(1) - 1).max() <= 4 * U
    assert np.array_equal(c["face"], ms.pick64(c["cdf"], c["u"][:, 0])) and np.all(c["areas"][c["face"]] > 0)
    pts, bound, n64 = ms.sample64(c["verts"], c["faces"], c["face"], b)
    err = np.abs(c["pts"] - pts)
    print(f"{name}: point error / bound max {np.max(err / np.maximum(bound, 1e-300)):.3f}")
    assert np.all(err <= bound)
    length = np.linalg.norm(c["nrm"].astype(F64), axis=1)
    assert np.abs(length - 1).max() <= 4 * U and np.all((c["nrm"] * n64).sum(1) > 0.999)


def test_a_degenerate_face_has_the_zero_normal_and_a_bad_face_is_not_loaded():
    verts, faces = ms.degenerate_mesh()
    only = faces[[3, 5]]                                      # collinear corners, one corner three times: both of area zero
    cdf = np.array([0, 0], F32)
    pts, nrm, face, flag = ms.host_sample(verts, only, cdf, np.random.default_rng(2).random((5, 3), dtype=F32))
    assert flag == 0 and np.all(face == 1) and np.all(nrm == 0) and np.abs(pts - verts[4]).max() <= 8 * U * np.abs(verts[4]).max()
    bad = faces.copy()
    bad[4] = (2, 12, 4)                                       # one past the last vertex
    areas, flag = ms.host_areas(verts, bad)
    assert flag == 1 and areas[4] == 0 and ms.same_bits(np.delete(areas, 4), np.delete(ms.host_areas(verts, faces)[0], 4))
    cdf = np.cumsum(ms.host_areas(verts, faces)[0], dtype=F32)
    u = np.zeros((64, 3), F32)
    u[:, 0] = np.arange(64, dtype=F32) / 64
    pts, nrm, face, flag = ms.host_sample(verts, bad, cdf, u)
    hit = face == 4
    assert flag == 1 and hit.any() and np.all(pts[hit] == 0) and np.all(nrm[hit] == 0)
    good = ms.host_sample(verts, faces, cdf, u)
    assert ms.same_bits(pts[~hit], good[0][~hit]) and ms.same_bits(nrm[~hit], good[1][~hit]) and np.array_equal(face, good[2])


# ----------------------------------------------------------------------------- reduction
@pytest.mark.parametrize("normals", [False, True], ids=["plain", "normals"])
@pytest.mark.parametrize("T", ms.SCORE_T)
@pytest.mark.parametrize("N", ms.SCORE_N)
def test_sums_against_float64(N, T, normals):
    c = ms.score_case(N, T, normals)
    want, bound = ms.score64(c["d2"], c["idx"], c["nq"], c["nr"], c["tau"])
    got = c["out"]
    assert np.array_equal(got[3:], want[3:])                                   # N and the counts: exact
    assert np.all(np.abs(got[:3] - want[:3]) <= bound[:3]), (got[:3] - want[:3], bound[:3])
    assert (got[2] > 0) == normals
    if T == 8 and N >= 64:
        assert got[4] >= np.count_nonzero(c["d2"] == F32(0.0625)) > 0          # tau = 0.25 counts sqrt(0.0625) = 0.25: "<="
        assert got[5] == np.count_nonzero(c["d2"] == 0) > 0                    # tau = 0: exactly the zeros


def test_idx_is_clamped_before_it_reads_a_normal():
    c = ms.score_case(65, 1, True)
    wild = c["idx"].copy()
    wild[3], wild[9] = -5, 10 ** 6
    ref = c["idx"].copy()
    ref[3], ref[9] = 0, len(c["nr"]) - 1
    assert ms.same_bits(ms.host_score(c["d2"], wild, c["nq"], c["nr"], c["tau"]), ms.host_score(c["d2"], ref, c["nq"], c["nr"], c["tau"]))


# ----------------------------------------------------------------------------- arguments
def test_the_restatement_rejects_sizes_of_zero_and_nine_thresholds():
    lib = ms.host_lib()
    buf = np.full(64, ms.SENTINEL, F32)
    untouched = buf.copy()
    p = buf.ctypes.data
    assert lib.ref_face_areas(p, 0, p, 4, p, p) == EINVAL and lib.ref_face_areas(p, 4, p, 0, p, p) == EINVAL
    assert lib.ref_face_areas(p, (1 << 24) + 1, p, 4, p, p) == EINVAL and lib.ref_face_areas(p, 4, p, 4, p, None) == EINVAL
    for V, Fc, M in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (1, 1, (1 << 24) + 1)):
        assert lib.ref_sample(p, V, p, Fc, p, p, M, p, p, p, p) == EINVAL
    for Nq, Nr in ((0, 5), (5, 0), (-1, 5), ((1 << 24) + 1, 5)):
        assert lib.ref_nearest(p, Nq, p, Nr, p, p) == EINVAL and lib.ref_nearest_workspace(Nq, Nr) == 0
    assert lib.ref_score(p, p, None, None, 0, 0, p, 1, p) == EINVAL and lib.ref_score(p, p, None, None, 0, 5, p, 9, p) == EINVAL
    assert lib.ref_score(p, p, p, None, 5, 5, p, 1, p) == EINVAL and lib.ref_score(p, p, p, p, 0, 5, p, 1, p) == EINVAL
    assert lib.ref_score(p, p, None, None, 0, 5, None, 1, p) == EINVAL and lib.ref_score(p, p, None, None, 0, 5, p, -1, p) == EINVAL
    assert ms.same_bits(buf, untouched)
    t = ms.tile()
    assert lib.ref_splits(1000, t) == 1 and lib.ref_splits(1000, t + 1) == 2 and lib.ref_splits(1000, 3 * t + 7) == 4
    assert lib.ref_splits(100_000, 100_000) > 1 and lib.ref_splits(1 << 24, 1 << 24) == 1
    assert lib.ref_nearest_workspace(1000, t) == 256 and lib.ref_nearest_workspace(1000, t + 1) == 256 + 8000


def test_the_entry_points_reject_the_same_before_any_launch():
    """the library's own entries (no GPU: each returns before a launch; ADDR is a host address no check follows)"""
    import core.mesh_score as cms
    cms.lib()
    p = ctypes.c_void_p(ADDR)
    areas, sample, nearest, score = (entry(n) for n in (ENTRIES[0], ENTRIES[1], ENTRIES[3], ENTRIES[4]))
    ws_bytes = entry(ENTRIES[2])
    assert areas(p, 0, p, 4, p, p, None) == EINVAL and areas(p, 4, p, 0, p, p, None) == EINVAL and areas(p, 4, p, 4, p, None, None) == EINVAL
    for V, Fc, M in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (1, 1, (1 << 24) + 1)):
        assert sample(p, V, p, Fc, p, p, M, p, p, p, p, None) == EINVAL
    for Nq, Nr in ((0, 5), (5, 0), (-1, 5), ((1 << 24) + 1, 5)):
        assert nearest(p, Nq, p, Nr, p, p, p, None) == EINVAL and ws_bytes(Nq, Nr) == 0
    assert nearest(p, 5, p, 5, p, p, None, None) == EINVAL
    assert score(p, p, None, None, 0, 0, p, 1, p, p, None) == EINVAL and score(p, p, None, None, 0, 5, p, 9, p, p, None) == EINVAL
    assert score(p, p, p, None, 5, 5, p, 1, p, p, None) == EINVAL and score(p, p, None, None, 0, 5, p, 1, p, None, None) == EINVAL
    lib = ms.host_lib()
    for Nq, Nr in ((1, 1), (1000, ms.tile()), (1000, ms.tile() + 1), (100_000, 100_000), (1 << 24, 1 << 24)):
        assert ws_bytes(Nq, Nr) == lib.ref_nearest_workspace(Nq, Nr) > 0


# ----------------------------------------------------------------------------- the header
def test_the_header_binds_as_a_satellite_and_the_library_exports_it():
    import os
    from core import _hip
    import core.mesh_score as cms
    path = os.path.join(os.path.dirname(_hip.HEADER_PATH), "danbo_mesh_score.h")
    bound = _hip.bind_headers([_hip.header(n).path for n in _hip.HEADERS] + [path])      # raises on a clash or a struct
    assert len(bound) == len(_hip.HEADERS) + 1 and bound[-1].path == path and not bound[-1].structs
    assert set(bound[-1].signatures) == set(ENTRIES) and "danbo_mesh_score.h" not in _hip.HEADERS
    assert all(n.startswith(("danbo_mesh_face_areas", "danbo_mesh_sample", "danbo_points_")) for n in bound[-1].signatures)
    assert bound[-1].restypes["danbo_points_nearest_workspace_bytes"] is ctypes.c_size_t
    assert vars(bound[-1].C) == dict(DANBO_POINTS_TILE=ms.tile(), DANBO_POINTS_MAX_TAU=ms.MAX_TAU, DANBO_POINTS_SCORE_WORKSPACE_BYTES=5888)
    assert cms.header().signatures == bound[-1].signatures and cms.TILE == ms.tile()
    l = cms.lib()
    assert l is _hip.lib() and l.danbo_abi_version() == 9
    for name, argtypes in bound[-1].signatures.items():
        fn = getattr(l, name)                                                             # AttributeError: not exported
        assert fn.argtypes == argtypes and fn.restype is bound[-1].restypes[name]


def test_tensors_off_the_device_raise():
    import torch
    import core.mesh_score as cms
    v, f = torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32)
    for call in (lambda: cms.face_areas(v, f), lambda: cms.sample_surface(v, f, 4), lambda: cms.nearest(v, v),
                 lambda: cms.score_points(v, None, v, None), lambda: cms.direction_sums(torch.zeros(3), f[:, 0], None, None, (0.1,))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
