"""Mesh scores on the GPU (csrc/k_mesh_score.hip through core/mesh_score.py, run_render --mesh_score, score_mesh.py): every kernel
against the serial restatement of csrc/mesh_score_math.hpp bit for bit, with guard words around what it writes, and the entry
points end to end against the restatement chained on the same samples."""
import ctypes
import os

import numpy as np
import pytest
import torch

import mesh_score_ref as ms
from helpers import ROOT, N, T, entry, same_bits
from mesh_score_ref import F32, F64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64                      # guard words on each side of an output
GUARD_BYTES = 512               # guard bytes on each side of a workspace


def cms():
    import core.mesh_score as m
    m.lib()
    return m


def guarded(n, dtype, fill):
    """a device buffer of GUARD + n + GUARD elements filled with `fill` -> (buffer, its middle n elements)"""
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def guards_intact(buf, fill):
    return bool((buf[:GUARD] == fill).all() and (buf[-GUARD:] == fill).all())


def P(t):
    return ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def gpu_nearest(q, r):
    """danbo_points_nearest through the C entry with guard words around d2, idx and the workspace -> (d2, idx, workspace bytes)"""
    cms()
    Nq, Nr = len(q), len(r)
    qt, rt = T(q), T(r)
    d2_buf, d2 = guarded(Nq, torch.float32, -777.25)
    idx_buf, idx = guarded(Nq, torch.int32, -7)
    nbytes = int(entry("danbo_points_nearest_workspace_bytes")(Nq, Nr))
    assert nbytes == ms.host_lib().ref_nearest_workspace(Nq, Nr) >= 256
    ws = torch.full((nbytes + 2 * GUARD_BYTES,), 0xA5, dtype=torch.uint8, device=DEV)
    rc = entry("danbo_points_nearest")(P(qt), Nq, P(rt), Nr, P(d2), P(idx), ctypes.c_void_p(ws.data_ptr() + GUARD_BYTES), stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert guards_intact(d2_buf, -777.25) and guards_intact(idx_buf, -7)
    assert bool((ws[:GUARD_BYTES] == 0xA5).all() and (ws[-GUARD_BYTES:] == 0xA5).all())
    return N(d2), N(idx), nbytes


# ----------------------------------------------------------------------------- nearest point
@pytest.mark.parametrize("Nr", ms.nearest_nr())
def test_nearest_equals_the_restatement_bitwise(Nr):
    tile = cms().TILE
    assert tile == ms.tile()
    for Nq in ms.NEAREST_NQ:
        c = ms.nearest_case(Nq, Nr)
        d2, idx, nbytes = gpu_nearest(c["q"], c["r"])
        assert (nbytes > 256) == (Nr > tile) == (ms.host_lib().ref_splits(Nq, Nr) > 1)      # the split path, and the one without
        assert same_bits(d2, c["d2"]) and same_bits(idx, c["idx"]), (Nq, Nr)


@pytest.mark.parametrize("Nr_tiles", [1, 3], ids=["one_launch", "split"])
def test_nearest_with_duplicates_and_with_itself(Nr_tiles):
    Nr = Nr_tiles * ms.tile() + (7 if Nr_tiles > 1 else 0)
    c = ms.nearest_case(1000, Nr, "duplicates")
    d2, idx, _ = gpu_nearest(c["q"], c["r"])
    assert same_bits(d2, c["d2"]) and same_bits(idx, c["idx"])
    r = c["r"]
    assert all(np.flatnonzero((r == r[j]).all(1))[0] == j for j in idx[:100])              # the lower index of equal points
    c = ms.nearest_case(1000, Nr, "self")
    d2, idx, _ = gpu_nearest(c["q"], c["r"])
    assert same_bits(d2, np.zeros(1000, F32)) and np.array_equal(idx, np.arange(1000)) and same_bits(idx, c["idx"])


def test_nearest_through_the_wrapper_twice():
    m = cms()
    c = ms.nearest_case(1000, 3 * ms.tile() + 7)
    q, r = T(c["q"]), T(c["r"])
    for _ in range(2):
        d2, idx = m.nearest(q, r)
        assert d2.dtype == torch.float32 and idx.dtype == torch.int32 and d2.is_cuda
        assert same_bits(N(d2), c["d2"]) and same_bits(N(idx), c["idx"])
    with pytest.raises(ValueError):
        m.nearest(q[:0], r)
    with pytest.raises(ValueError):
        m.nearest(q, r[:, :2])


# ----------------------------------------------------------------------------- areas and samples
@pytest.mark.parametrize("name", sorted(ms.MESHES))
def test_areas_and_samples_equal_the_restatement_bitwise(name):
    m = cms()
    for M in ms.SAMPLE_M:
        c = ms.sample_case(name, M)
        verts, faces = T(c["verts"]), T(c["faces"], torch.int32)
        F = len(c["faces"])
        a_buf, areas = guarded(F, torch.float32, -777.25)
        flag = torch.zeros(1, dtype=torch.int32, device=DEV)
        assert entry("danbo_mesh_face_areas")(P(verts), len(c["verts"]), P(faces), F, P(areas), P(flag), stream()) == 0
        bufs = [guarded(3 * M, torch.float32, -777.25), guarded(3 * M, torch.float32, -777.25), guarded(M, torch.int32, -7)]
        cdf, u = T(c["cdf"]), T(c["u"])
        assert entry("danbo_mesh_sample")(P(verts), len(c["verts"]), P(faces), F, P(cdf), P(u), M, P(bufs[0][1]), P(bufs[1][1]),
                                          P(bufs[2][1]), P(flag), stream()) == 0
        torch.cuda.synchronize()
        assert int(flag.item()) == 0 and guards_intact(a_buf, -777.25) and same_bits(N(areas), c["areas"])
        assert all(guards_intact(b, fill) for (b, _), fill in zip(bufs, (-777.25, -777.25, -7)))
        assert same_bits(N(bufs[0][1]).reshape(M, 3), c["pts"]) and same_bits(N(bufs[1][1]).reshape(M, 3), c["nrm"])
        assert same_bits(N(bufs[2][1]), c["face"])
        pts, nrm, face = m.sample_with(verts, faces, cdf, u)
        assert same_bits(N(pts), c["pts"]) and same_bits(N(nrm), c["nrm"]) and same_bits(N(face), c["face"])
        assert same_bits(N(m.face_areas(verts, faces)), c["areas"])


def test_a_face_index_out_of_range_raises():
    """the kernels check the three corner indices of a face before they load through them (mesh_face_corners: 0 <= i < V, else the
    face is skipped and the flag set), so the bad face is an argument the wrapper reports, not a load"""
    m = cms()
    verts, faces = ms.degenerate_mesh()
    for corner in (12, -1, 2 ** 31 - 1):
        bad = faces.copy()
        bad[4, 1] = corner
        with pytest.raises(ValueError, match="outside the vertex array"):
            m.face_areas(T(verts), T(bad, torch.int32))
        with pytest.raises(ValueError, match="outside the vertex array"):
            m.sample_surface(T(verts), T(bad, torch.int32), 256)
        # the kernels' own outputs on the bad mesh are the restatement's: +0 for the face, the flag set, the rest untouched by it
        cdf = np.cumsum(ms.host_areas(verts, faces)[0], dtype=F32)
        u = np.zeros((64, 3), F32)
        u[:, 0] = np.arange(64, dtype=F32) / 64
        want = ms.host_sample(verts, bad, cdf, u)
        out = [torch.empty(192, device=DEV), torch.empty(192, device=DEV), torch.empty(64, dtype=torch.int32, device=DEV)]
        flag = torch.zeros(1, dtype=torch.int32, device=DEV)
        tv, tf, tc, tu = T(verts), T(bad, torch.int32), T(cdf), T(u)
        assert entry("danbo_mesh_sample")(P(tv), 12, P(tf), len(bad), P(tc), P(tu), 64, P(out[0]), P(out[1]), P(out[2]), P(flag), stream()) == 0
        torch.cuda.synchronize()
        assert int(flag.item()) == 1 == want[3] and (want[2] == 4).any()
        assert same_bits(N(out[0]).reshape(64, 3), want[0]) and same_bits(N(out[1]).reshape(64, 3), want[1]) and same_bits(N(out[2]), want[2])


# ----------------------------------------------------------------------------- sums
@pytest.mark.parametrize("normals", [False, True], ids=["plain", "normals"])
@pytest.mark.parametrize("n_tau", ms.SCORE_T)
def test_sums_equal_the_restatement_bitwise(n_tau, normals):
    m = cms()
    for n in ms.SCORE_N:
        c = ms.score_case(n, n_tau, normals)
        d2, idx, tau = T(c["d2"]), T(c["idx"], torch.int32), T(c["tau"])
        nq, nr = (T(c["nq"]), T(c["nr"])) if normals else (None, None)
        out_buf, out = guarded(4 + n_tau, torch.float64, -777.25)
        nbytes = m.header().C.DANBO_POINTS_SCORE_WORKSPACE_BYTES
        ws = torch.full((nbytes + 2 * GUARD_BYTES,), 0xA5, dtype=torch.uint8, device=DEV)
        rc = entry("danbo_points_score")(P(d2), P(idx), None if nq is None else P(nq), None if nr is None else P(nr),
                                         len(c["nr"]) if normals else 0, n, P(tau), n_tau, P(out),
                                         ctypes.c_void_p(ws.data_ptr() + GUARD_BYTES), stream())
        torch.cuda.synchronize()
        assert rc == 0 and guards_intact(out_buf, -777.25)
        assert bool((ws[:GUARD_BYTES] == 0xA5).all() and (ws[-GUARD_BYTES:] == 0xA5).all())
        assert same_bits(N(out), np.asarray(c["out"])), (n, N(out), c["out"])
        assert same_bits(N(m.direction_sums(d2, idx, nq, nr, c["tau"].tolist())), np.asarray(c["out"]))


# ----------------------------------------------------------------------------- end to end
def test_score_meshes_of_two_icospheres_equals_the_chained_restatement():
    m = cms()
    a, b = ms.icosphere(2, 1.0), ms.icosphere(2, 1.1)
    ta, tb = (T(a[0]), T(a[1], torch.int32)), (T(b[0]), T(b[1], torch.int32))
    n, taus, seed = 1500, (0.05, 0.15, 0.4), 3
    got = m.score_meshes(ta, tb, n_points=n, thresholds=taus, seed=seed)
    inputs = []
    for mesh in (ta, tb):
        gen = torch.Generator(device=DEV)
        gen.manual_seed(seed)
        cdf, u = m.sample_inputs(*mesh, n, gen)
        inputs.append((N(cdf), N(u)))
    ab, ba, _ = ms.host_chain(a, *inputs[0], b, *inputs[1], taus)
    want = ms.metrics64(ab, ba, taus)
    print("two icospheres:", got)
    assert got == want
    # the surfaces are 0.1 apart at the vertices and at most 0.1 + the sagitta of a face elsewhere
    # (1500 samples of an area of 4 pi r^2 lie ~0.1 apart: a nearest sample is found within 0.4 of every sample, none within 0.05)
    assert 0.09 < got["chamfer_l1"] < 0.2 and got["fscore"][0.05] == 0 and got["fscore"][0.4] == 1 and got["normal_consistency"] > 0.9
    same = m.score_meshes(ta, ta, n_points=n, thresholds=taus, seed=seed)
    assert same["chamfer_l1"] == 0 and same["chamfer_l2"] == 0 and all(v == 1 for v in same["fscore"].values())
    assert abs(same["normal_consistency"] - 1) < 1e-6
    other = m.score_meshes(ta, ta, n_points=n, thresholds=taus, seed=(3, 4))
    assert 0 < other["chamfer_l1"] < 0.1


def test_run_render_scores_its_meshes_and_score_mesh_pairs_files(tmp_path):
    import run_nerf
    import run_render
    import score_mesh
    from core.utils.mesh_io import read_ply
    m = cms()
    cfg = os.path.join(ROOT, "danbo-pytorch_amd", "configs", "surreal", "danbo_fast.txt")
    run_nerf.train(["--config", cfg, "--basedir", str(tmp_path), "--expname", "demo", "--syn_poses", "2", "--syn_cams", "2",
                    "--syn_res", "32", "--syn_rest_scale", "0.714", "--N_rand", "512", "--N_sample_images", "4", "--i_print", "10",
                    "--i_weights", "20", "--i_testset", "20", "--render_factor", "0", "--n_iters", "20"])
    log = tmp_path / "demo"
    probe = ["--nerf_args", str(log / "args.txt"), "--ckptpath", str(log / "000020.tar"), "--dataset", "synthetic", "--entry", "val",
             "--outputdir", str(tmp_path / "out"), "--render_type", "selected", "--selected_idxs", "1", "--render_mesh", "--mesh_res", "31",
             "--mesh_radius", "1.2"]
    run_render.run_render(probe + ["--runname", "probe"])
    sig = np.load(tmp_path / "out" / "probe" / "meshes" / "000_sigma.npy")
    thr = repr(float(F32(np.median(sig[sig > 0]))))             # a threshold the 20-step network does reach
    base = probe + ["--mesh_threshold", thr]
    run_render.run_render(base + ["--runname", "plain"])
    plain = tmp_path / "out" / "plain"
    assert not any(n.startswith("mesh_score") for n in os.listdir(plain)) and sorted(os.listdir(plain / "meshes")) == ["000.ply", "000_sigma.npy"]
    n, taus = 2000, (0.25, 0.5)
    run_render.run_render(base + ["--runname", "scored", "--mesh_score", str(plain / "meshes"), "--mesh_score_points", str(n),
                                  "--mesh_score_tau"] + [repr(t) for t in taus])
    scored = tmp_path / "out" / "scored"
    # what the run wrote before the flag existed is what it writes with and without it, byte for byte
    for name in ("000.ply", "000_sigma.npy"):
        assert (scored / "meshes" / name).read_bytes() == (plain / "meshes" / name).read_bytes()
    assert set(os.listdir(scored)) - set(os.listdir(plain)) == {"mesh_score_final.txt", "mesh_scores.npy"}
    table = np.load(scored / "mesh_scores.npy")
    cols = m.score_columns(taus)
    assert table.shape == (1, 4 + 3 * len(taus)) and table.dtype == F64 and len(cols) == table.shape[1]
    row = dict(zip(cols, table[0]))
    # the float64 statement on the same samples: the mesh against itself, sampled with seeds 0 and 1
    v, f = read_ply(str(plain / "meshes" / "000.ply"))
    pts = []
    for seed in (0, 1):
        gen = torch.Generator(device=DEV)
        gen.manual_seed(seed)
        cdf, u = m.sample_inputs(T(v), T(f, torch.int32), n, gen)
        pts.append(ms.host_sample(v, f, N(cdf), N(u))[0])
    d_ab, d_ba = np.sqrt(ms.nearest64(pts[0], pts[1])[0]), np.sqrt(ms.nearest64(pts[1], pts[0])[0])
    spacing, mean64 = max(d_ab.max(), d_ba.max()), 0.5 * (d_ab.mean() + d_ba.mean())
    print("run_render --mesh_score:", row, "float64 chamfer_l1", mean64, "largest nearest distance", spacing)
    assert 0 < row["chamfer_l1"] <= spacing and abs(row["chamfer_l1"] - mean64) <= 4 * ms.U * mean64
    assert spacing <= taus[0] and all(row[f"fscore@{t:g}"] == 1 for t in taus) and row["n_points"] == n
    text = (scored / "mesh_score_final.txt").read_text().splitlines()
    assert [line.split(":")[0] for line in text] == cols and float(text[0].split(":")[1]) == row["chamfer_l1"]
    # a missing file is an error that names it
    empty = tmp_path / "nothing"
    empty.mkdir()
    with pytest.raises(FileNotFoundError, match="000.ply"):
        run_render.run_render(base + ["--runname", "missing", "--mesh_score", str(empty)])
    # score_mesh.py: the same numbers for the files on disk
    names, t2 = score_mesh.main(["--pred", str(scored / "meshes"), "--gt", str(plain / "meshes"), "--out", str(tmp_path / "tables"),
                                 "--points", str(n), "--tau"] + [repr(t) for t in taus])
    assert names == ["000.ply"] and same_bits(t2, table) and same_bits(np.load(tmp_path / "tables" / "mesh_scores.npy"), table)
    with pytest.raises(FileNotFoundError, match="000.ply"):
        score_mesh.main(["--pred", str(scored / "meshes"), "--gt", str(empty)])
