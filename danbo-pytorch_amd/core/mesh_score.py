"""Scores of triangle meshes on the device (include/danbo_mesh_score.h, csrc/k_mesh_score.hip; the definitions are stated once in
csrc/mesh_score_math.hpp): area-weighted surface samples, the exact nearest neighbour between two point sets, and Chamfer distance,
F-score and normal consistency from the 4 + T float64 sums of each direction -- the only numbers that cross to the host.

The header is a satellite that _hip.HEADERS does not list yet: it is bound here, once, with the public call that binds the table
(so the rule "no struct, no name an earlier header declares" holds for it too), and the types of its entries are set on the handle
of _hip.lib()."""
import os

import numpy as np
import torch

from . import _hip

HEADER = "danbo_mesh_score.h"
_bound = None
_typed = False


def header():
    """what include/danbo_mesh_score.h declares: .path, .signatures, .restypes, .C -- bound beside every header of _hip.HEADERS"""
    global _bound
    if _bound is None:
        path = os.path.join(os.path.dirname(_hip.HEADER_PATH), HEADER)
        _bound = _hip.bind_headers([_hip.header(n).path for n in _hip.HEADERS] + [path])[-1]
    return _bound


def lib():
    """_hip.lib() with the types of this header's entries set (a library that lacks one is stale)"""
    global _typed
    l = _hip.lib()
    if not _typed:
        h = header()
        for name, argtypes in h.signatures.items():
            fn = getattr(l, name, None)
            if fn is None:
                raise RuntimeError(f"{_hip.LIB_PATH} has no {name}, which {h.path} declares: "
                                   "the library is stale, rebuild it with `make -C danbo-pytorch_amd/csrc`")
            fn.argtypes = argtypes
            fn.restype = h.restypes[name]
        _typed = True
    return l


TILE = header().C.DANBO_POINTS_TILE          # reference points per LDS tile of danbo_points_nearest
MAX_TAU = header().C.DANBO_POINTS_MAX_TAU
MAX_SIZE = 1 << 24


def _call(name, *args):
    _hip.check(getattr(lib(), name)(*args), name)


def _device(t, name, who, dtype, cols=None):
    """t as the kernels read it: a contiguous device tensor of `dtype`, [n, cols] (cols None: [n]) with 1 <= n <= 2^24"""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{who}: {name}: expected a CUDA/HIP tensor -- libdanbo_hip has no CPU fallback")
    shape_ok = t.dim() == 1 if cols is None else (t.dim() == 2 and t.shape[1] == cols)
    if t.dtype != dtype or not shape_ok:
        raise ValueError(f"{who}: {name} must be a {dtype} tensor of shape [n{'' if cols is None else f', {cols}'}]")
    if not 1 <= t.shape[0] <= MAX_SIZE:
        raise ValueError(f"{who}: {name} must hold 1 .. 2^24 rows, not {t.shape[0]}")
    return t.contiguous()


def _mesh(verts, faces, who):
    verts = _device(verts, "verts", who, torch.float32, 3)
    faces = _device(faces, "faces", who, torch.int32, 3)
    if faces.device != verts.device:
        raise RuntimeError(f"{who}: faces: expected a tensor on {verts.device}")
    return verts, faces


def _raise_bad_face(flag, who):
    if int(flag.max().item()) != 0:
        raise ValueError(f"{who}: a face index lies outside the vertex array")


def _face_areas(verts, faces, flag):
    areas = torch.empty(faces.shape[0], device=verts.device, dtype=torch.float32)
    with torch.cuda.device(verts.device):
        _call("danbo_mesh_face_areas", _hip.ptr(verts), verts.shape[0], _hip.ptr(faces), faces.shape[0], _hip.ptr(areas), _hip.ptr(flag),
              _hip.stream())
    return areas


def face_areas(verts, faces):
    """danbo_mesh_face_areas: verts [V,3] float32, faces [F,3] int32 on the device -> areas [F] float32.  ValueError for a face index
    outside the vertex array (the kernel does not load through it)."""
    verts, faces = _mesh(verts, faces, "face_areas")
    flag = torch.zeros(1, device=verts.device, dtype=torch.int32)
    areas = _face_areas(verts, faces, flag)
    _raise_bad_face(flag, "face_areas")
    return areas


def sample_with(verts, faces, cdf, u):
    """danbo_mesh_sample on a given cdf [F] and u [M,3] (both float32 on the device) -> pts [M,3], normals [M,3], face [M] int32"""
    who = "sample_with"
    verts, faces = _mesh(verts, faces, who)
    cdf = _device(cdf, "cdf", who, torch.float32)
    u = _device(u, "u", who, torch.float32, 3)
    if cdf.shape[0] != faces.shape[0] or cdf.device != verts.device or u.device != verts.device:
        raise ValueError(f"{who}: cdf must hold one value per face, and cdf and u lie on {verts.device}")
    M = u.shape[0]
    pts = torch.empty(M, 3, device=verts.device, dtype=torch.float32)
    nrm = torch.empty(M, 3, device=verts.device, dtype=torch.float32)
    face = torch.empty(M, device=verts.device, dtype=torch.int32)
    flag = torch.zeros(1, device=verts.device, dtype=torch.int32)
    with torch.cuda.device(verts.device):
        _call("danbo_mesh_sample", _hip.ptr(verts), verts.shape[0], _hip.ptr(faces), faces.shape[0], _hip.ptr(cdf), _hip.ptr(u), M,
              _hip.ptr(pts), _hip.ptr(nrm), _hip.ptr(face), _hip.ptr(flag), _hip.stream())
    _raise_bad_face(flag, who)
    return pts, nrm, face


def sample_inputs(verts, faces, n, generator=None):
    """(cdf [F], u [n,3]) of sample_surface: the cumulative sum of the device areas and torch.rand on the device"""
    verts, faces = _mesh(verts, faces, "sample_surface")
    if not 1 <= int(n) <= MAX_SIZE:
        raise ValueError(f"sample_surface: 1 .. 2^24 samples, not {n}")
    cdf = torch.cumsum(face_areas(verts, faces), 0)
    u = torch.rand(int(n), 3, device=verts.device, dtype=torch.float32, generator=generator)
    return cdf, u


def sample_surface(verts, faces, n, generator=None):
    """n points of the surface, uniform by area -> pts [n,3], normals [n,3] (the faces' unit normals), face [n] int32, all on the
    device.  generator: a torch.Generator of the mesh's device."""
    cdf, u = sample_inputs(verts, faces, n, generator)
    return sample_with(verts, faces, cdf, u)


def nearest(q, r):
    """danbo_points_nearest: q [Nq,3], r [Nr,3] float32 on the device -> d2 [Nq] float32 (the squared distance to the nearest point
    of r), idx [Nq] int32 (its index; the lowest among equals).  Exact: every pair is evaluated."""
    who = "nearest"
    q = _device(q, "q", who, torch.float32, 3)
    r = _device(r, "r", who, torch.float32, 3)
    if r.device != q.device:
        raise RuntimeError(f"{who}: r: expected a tensor on {q.device}")
    Nq, Nr = q.shape[0], r.shape[0]
    d2 = torch.empty(Nq, device=q.device, dtype=torch.float32)
    idx = torch.empty(Nq, device=q.device, dtype=torch.int32)
    ws = torch.empty(int(lib().danbo_points_nearest_workspace_bytes(Nq, Nr)), device=q.device, dtype=torch.uint8)
    with torch.cuda.device(q.device):
        _call("danbo_points_nearest", _hip.ptr(q), Nq, _hip.ptr(r), Nr, _hip.ptr(d2), _hip.ptr(idx), _hip.ptr(ws), _hip.stream())
    return d2, idx


def direction_sums(d2, idx, nq, nr, thresholds):
    """danbo_points_score: the 4 + T float64 numbers of one direction, on the device: sum d, sum d2, sum |n . m|, N, counts"""
    who = "direction_sums"
    d2 = _device(d2, "d2", who, torch.float32)
    idx = _device(idx, "idx", who, torch.int32)
    N = d2.shape[0]
    if idx.shape[0] != N or idx.device != d2.device:
        raise ValueError(f"{who}: idx must hold one index per distance, on {d2.device}")
    if (nq is None) != (nr is None):
        raise ValueError(f"{who}: normals of both sets or of neither")
    if nq is not None:
        nq, nr = _device(nq, "nq", who, torch.float32, 3), _device(nr, "nr", who, torch.float32, 3)
        if nq.shape[0] != N or nq.device != d2.device or nr.device != d2.device:
            raise ValueError(f"{who}: nq must hold one normal per query, and both normal sets lie on {d2.device}")
    tau = [float(t) for t in thresholds]
    if len(tau) > MAX_TAU:
        raise ValueError(f"{who}: at most {MAX_TAU} thresholds, not {len(tau)}")
    T = len(tau)
    tau_t = torch.tensor(tau or [0.], device=d2.device, dtype=torch.float32)
    out = torch.empty(4 + T, device=d2.device, dtype=torch.float64)
    ws = torch.empty(header().C.DANBO_POINTS_SCORE_WORKSPACE_BYTES, device=d2.device, dtype=torch.uint8)
    with torch.cuda.device(d2.device):
        _call("danbo_points_score", _hip.ptr(d2), _hip.ptr(idx), _hip.ptr(nq), _hip.ptr(nr), 0 if nr is None else nr.shape[0], N,
              _hip.ptr(tau_t), T, _hip.ptr(out), _hip.ptr(ws), _hip.stream())
    return out


def scores_from_sums(ab, ba, thresholds):
    """the dict of score_points from the two directions' 4 + T numbers (host sequences): ab = a's points against b, ba = b's
    against a.  precision is the share of a's points within tau of b, recall the share of b's points within tau of a."""
    ab, ba = [float(x) for x in ab], [float(x) for x in ba]
    na, nb = ab[3], ba[3]
    out = dict(chamfer_l1=0.5 * (ab[0] / na + ba[0] / nb), chamfer_l2=ab[1] / na + ba[1] / nb,
               normal_consistency=0.5 * (ab[2] / na + ba[2] / nb), precision={}, recall={}, fscore={})
    for t, tau in enumerate(thresholds):
        p, r = ab[4 + t] / na, ba[4 + t] / nb
        out["precision"][tau], out["recall"][tau] = p, r
        out["fscore"][tau] = 2 * p * r / (p + r) if p + r > 0 else 0.0
    return out


def score_points(pa, na, pb, nb, thresholds=(0.01, 0.02)):
    """Two point sets pa [Na,3], pb [Nb,3] with their unit normals na, nb (both or neither None), float32 on the device -> dict of
    chamfer_l1 = 0.5 (mean_a d + mean_b d), chamfer_l2 = mean_a d^2 + mean_b d^2, precision[tau], recall[tau], fscore[tau] =
    2 P R / (P + R) (0 where P + R = 0) and normal_consistency = the mean of the two directions' mean |n . m| (0 without normals).
    `a` is the prediction: precision counts its points within tau of b.  One host read: the 2 x (4 + T) sums."""
    thresholds = tuple(float(t) for t in thresholds)
    d2_ab, i_ab = nearest(pa, pb)
    d2_ba, i_ba = nearest(pb, pa)
    sums = torch.stack([direction_sums(d2_ab, i_ab, na, nb, thresholds), direction_sums(d2_ba, i_ba, nb, na, thresholds)]).cpu().numpy()
    return scores_from_sums(sums[0], sums[1], thresholds)


def _load(mesh, device):
    if isinstance(mesh, (str, os.PathLike)):
        from .utils.mesh_io import read_ply
        v, f = read_ply(os.fspath(mesh))
        return torch.tensor(np.ascontiguousarray(v), device=device), torch.tensor(np.ascontiguousarray(f), device=device)
    verts, faces = mesh
    return verts, faces


def score_meshes(a, b, n_points=100_000, thresholds=(0.01, 0.02), seed=0, device=None):
    """a (the prediction), b (the ground truth): (verts [V,3] float32, faces [F,3] int32) on the device, or paths of .ply files
    (core.utils.mesh_io.read_ply; uploaded to `device`, default the current one).  n_points surface samples of each, drawn with a
    generator seeded `seed` for a and again `seed` for b -- the same mesh on both sides gets the same samples; seed = (seed_a,
    seed_b) draws the two sides differently --, then score_points with the faces' normals."""
    if not torch.cuda.is_available():
        raise RuntimeError("score_meshes: no GPU visible -- libdanbo_hip has no CPU fallback")
    dev = torch.device(device) if device is not None else next(
        (m[0].device for m in (a, b) if not isinstance(m, (str, os.PathLike)) and isinstance(m[0], torch.Tensor) and m[0].is_cuda),
        torch.device("cuda", torch.cuda.current_device()))
    sampled, seeds = [], tuple(seed) if isinstance(seed, (tuple, list)) else (seed, seed)
    for mesh, one_seed in zip((a, b), seeds):
        verts, faces = _load(mesh, dev)
        gen = torch.Generator(device=dev)
        gen.manual_seed(int(one_seed))
        sampled.append(sample_surface(verts, faces, n_points, generator=gen)[:2])
    (pa, na), (pb, nb) = sampled
    return score_points(pa, na, pb, nb, thresholds)


# ---- tables of scores (run_render.py --mesh_score, score_mesh.py) ----
def score_columns(thresholds):
    """the column names of a row of mesh_scores.npy: 4 + 3 T"""
    cols = ["chamfer_l1", "chamfer_l2", "normal_consistency", "n_points"]
    for tau in thresholds:
        cols += [f"precision@{tau:g}", f"recall@{tau:g}", f"fscore@{tau:g}"]
    return cols


def score_row(s, n_points, thresholds):
    row = [s["chamfer_l1"], s["chamfer_l2"], s["normal_consistency"], float(n_points)]
    for tau in thresholds:
        row += [s["precision"][tau], s["recall"][tau], s["fscore"][tau]]
    return row


def score_line(name, s, thresholds):
    f = " ".join(f"F@{tau:g} {s['fscore'][tau]:.4f}" for tau in thresholds)
    return f"mesh score {name}: chamfer_l1 {s['chamfer_l1']:.6f} chamfer_l2 {s['chamfer_l2']:.3e} {f} NC {s['normal_consistency']:.4f}"


def save_scores(basedir, rows, thresholds):
    """mesh_scores.npy [N, 4 + 3 T] float64 and mesh_score_final.txt (the column means) in basedir"""
    table = np.asarray(rows, np.float64).reshape(len(rows), 4 + 3 * len(thresholds))
    np.save(os.path.join(basedir, "mesh_scores.npy"), table)
    with open(os.path.join(basedir, "mesh_score_final.txt"), "w") as f:
        for name, v in zip(score_columns(thresholds), table.mean(0)):
            f.write(f"{name}: {v}\n")
    return table
