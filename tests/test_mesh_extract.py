"""Isosurface extraction (csrc/mesh_math.hpp, csrc/mc_table.inc, csrc/k_mesh.hip) on the CPU: the serial extractor -- the scalar
code the gfx950 kernels inline, compiled by g++ at test time -- against numpy predictions (never against itself): the vertices are
exactly the crossing edges in the defined order, every triangle lives on its own cell's edges, analytic surfaces come out closed,
oriented, with the right topology, distance and volume, white noise exercises all 256 cases, degenerate grids stay in bounds.
Plus the generated table, the .ply reader / writer and the host-side argument checks of the library."""
import ctypes
import os

import numpy as np
import pytest

import mesh_ref as m
from helpers import ROOT

F32 = np.float32
H = 1.0                                   # grid spacing of the analytic surfaces (index units)


def analytic_grids():
    return dict(sphere=m.sphere_grid(), torus=m.torus_grid(), two_spheres=m.two_spheres_grid(), clipped=m.sphere_grid(R=20.),
                noise0=m.noise_grid(0), noise1=m.noise_grid(1))


def more_grids():
    rng = np.random.default_rng(5)
    odd = rng.standard_normal((3, 5, 130)).astype(F32)
    box = (rng.standard_normal((9, 6, 7)) * 3).astype(F32)
    view = np.ascontiguousarray(rng.standard_normal((6, 9, 11)).astype(F32)).transpose(1, 0, 2)      # strides as render_mesh_density's
    return dict(odd=(odd, 0.25, -np.inf), floored=(box, 0.5, 0.), floored_iso0=(box, 0., 0.), view=(view, -0.1, -np.inf),
                tiny=(rng.standard_normal((2, 2, 2)).astype(F32), 0., -np.inf))


def all_cases():
    out = {k: (g, 0., -np.inf) for k, g in analytic_grids().items()}
    out.update(more_grids())
    return out


# ----------------------------------------------------------------------------- 1. vertices = crossing edges
@pytest.mark.parametrize("name", sorted(all_cases()))
def test_vertices_are_exactly_the_crossing_edges(name):
    """V = number of sign changes along the three axes; vertex k lies on the k-th crossing edge of the defined order (ascending by
    (linear index of the lower end) * 3 + axis), at the float64 evaluation of p + t e_ax within 3e-7 + 1.2e-7 |x| per coordinate:
    two rounded differences and one correctly rounded quotient (<= 1.8e-7 on t <= 1), half an ulp of the sum (<= 6e-8 |x|), doubled"""
    sigma, iso, floor = all_cases()[name]
    verts, faces = m.host_extract(sigma, iso, floor)
    inside, p, ax = m.crossing_edges(sigma, iso, floor)
    n_cross = sum(int((np.diff(inside, axis=a) != 0).sum()) for a in range(3))
    assert len(verts) == n_cross == len(p)
    pos, _, _ = m.vertex_positions_f64(sigma, iso, floor, p, ax)
    err = np.abs(verts.astype(np.float64) - pos)
    bound = 3e-7 + 1.2e-7 * np.abs(pos)
    print(name, "V", len(verts), "T", len(faces), "max err / bound", float((err / bound).max()) if len(verts) else 0.)
    assert np.all(err <= bound)
    # off the edge's axis the coordinates are the integers of the lower end, exactly
    off_axis = np.ones_like(pos, bool)
    off_axis[np.arange(len(p)), ax] = False
    assert np.array_equal(verts[off_axis], p[off_axis].astype(F32))
    assert faces.size == 0 or (faces.min() >= 0 and faces.max() < len(verts))


# ----------------------------------------------------------------------------- 2. triangles live on their own cell
@pytest.mark.parametrize("name", sorted(all_cases()))
def test_every_triangle_uses_three_edges_of_its_own_cell(name):
    """triangles come cell by cell in ascending linear cell index, as many per cell as the generated table has for the cell's
    numpy-computed case (<= 5); the three vertices of a triangle are distinct and lie on the twelve edges of that cell"""
    sigma, iso, floor = all_cases()[name]
    verts, faces = m.host_extract(sigma, iso, floor)
    inside, p, ax = m.crossing_edges(sigma, iso, floor)
    table = m.gen_table_module().TABLE
    ntri = np.array([len(t) for t in table])
    assert ntri.max() == 5 and ntri.sum() == 820
    cases = m.cell_cases(inside)
    per_cell = ntri[cases].ravel()
    assert len(faces) == per_cell.sum()
    cell = np.repeat(np.arange(per_cell.size), per_cell)
    cijk = np.stack(np.unravel_index(cell, cases.shape), -1)
    assert np.all((faces[:, 0] != faces[:, 1]) & (faces[:, 1] != faces[:, 2]) & (faces[:, 0] != faces[:, 2]))
    for c in range(3):
        lo = p[faces[:, c]] - cijk                        # lower end of the vertex' edge relative to the cell
        hi = lo.copy()
        hi[np.arange(len(hi)), ax[faces[:, c]]] += 1
        assert np.all((lo >= 0) & (lo <= 1) & (hi >= 0) & (hi <= 1))
    # and in table order: the edge (axis, corner) of every triangle corner is the table's
    gen = m.gen_table_module()
    want = np.array([e for cs in cases.ravel() for t in table[cs] for e in t], dtype=np.int64).reshape(-1, 3)
    lo = p[faces] - cijk[:, None, :]
    corner = lo[..., 0] + 2 * lo[..., 1] + 4 * lo[..., 2]
    got = np.vectorize(lambda a, c: gen.EDGE_ID[(c, c + (1 << a))])(ax[faces], corner) if len(faces) else want
    assert np.array_equal(got, want)


# ----------------------------------------------------------------------------- 3. analytic surfaces
def test_sphere_is_closed_oriented_and_as_round_as_linear_interpolation_allows():
    R = 9.2
    verts, faces = m.host_extract(m.sphere_grid(R=R), 0.)
    assert m.is_closed_oriented_manifold(faces)
    assert m.euler_characteristic(len(verts), faces) == 2
    r = np.linalg.norm(verts.astype(np.float64) - m.CENTRE, axis=1)
    inside_by, outside_by = float((R - r).max()), float((r - R).max())
    print("sphere: inside by", inside_by, "outside by", outside_by)
    # the field is concave along an edge: linear interpolation lands inside, by at most h^2 / (8 (R - 2h)) (+ 1e-5: the fp32 grid)
    assert inside_by <= H * H / (8 * (R - 2 * H)) + 1e-5 and outside_by <= 1e-5
    vol = m.signed_volume(verts, faces)
    deficit = 1. - vol / (4. / 3. * np.pi * R ** 3)
    print("sphere: signed volume", vol, "deficit", deficit)
    assert vol > 0                                         # normals point from inside (high density) to outside
    assert 0. <= deficit <= 1.5 * (H / R) ** 2


def test_torus_and_two_spheres_have_their_topology():
    verts, faces = m.host_extract(m.torus_grid(), 0.)
    assert m.is_closed_oriented_manifold(faces) and m.euler_characteristic(len(verts), faces) == 0
    assert m.signed_volume(verts, faces) > 0
    verts, faces = m.host_extract(m.two_spheres_grid(), 0.)
    assert m.is_closed_oriented_manifold(faces) and m.euler_characteristic(len(verts), faces) == 4
    assert m.signed_volume(verts, faces) > 0


def test_a_sphere_larger_than_the_grid_is_open_only_at_the_boundary():
    g = m.sphere_grid(R=20.)
    verts, faces = m.host_extract(g, 0.)
    assert len(faces) > 100
    de = m.directed_edges(faces)
    assert all(n == 1 for n in de.values())                # no undirected edge used more than twice, never twice the same way
    once = [e for e in de if (e[1], e[0]) not in de]
    assert once
    v = verts.astype(np.float64)
    on_boundary = np.any((v == 0.) | (v == np.array(g.shape) - 1.), axis=1)
    assert all(on_boundary[a] and on_boundary[b] for a, b in once)


# ----------------------------------------------------------------------------- 4. all 256 cases
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_white_noise_covers_all_cases_closed_and_oriented(seed):
    g = m.noise_grid(seed)
    verts, faces = m.host_extract(g, 0.)
    assert len(np.unique(m.cell_cases(g >= 0))) == 256
    de = m.directed_edges(faces)
    assert all(de.get((b, a), 0) == n for (a, b), n in de.items())         # every directed edge as often as its reverse
    doubled = sum(n for n in de.values() if n > 1)
    print("noise", seed, "directed edges", sum(de.values()), "of multiplicity > 1:", doubled)
    assert max(de.values()) <= 2 and doubled <= 1e-3 * sum(de.values())
    assert np.all((faces[:, 0] != faces[:, 1]) & (faces[:, 1] != faces[:, 2]) & (faces[:, 0] != faces[:, 2]))


# ----------------------------------------------------------------------------- 5. degenerate input
def _predicted_counts(sigma, iso, floor):
    inside, p, _ = m.crossing_edges(sigma, iso, floor)
    ntri = np.array([len(t) for t in m.gen_table_module().TABLE])
    return len(p), int(ntri[m.cell_cases(inside)].sum())


def test_degenerate_grids_stay_finite_and_in_bounds():
    rng = np.random.default_rng(11)
    const = np.full((5, 6, 7), F32(3.))
    wild = (rng.standard_normal((7, 8, 9)) * 4).astype(F32)
    flat = wild.ravel()
    flat[rng.choice(flat.size, 60, replace=False)] = np.nan
    flat[rng.choice(flat.size, 40, replace=False)] = np.inf
    flat[rng.choice(flat.size, 40, replace=False)] = -np.inf
    equal = rng.standard_normal((6, 6, 6)).astype(F32)
    equal[2:4, 2:4, 2:4] = F32(0.75)                       # a value equal to iso is inside
    cases = [("constant", const, 3.5, -np.inf), ("constant at iso", const, 3., -np.inf), ("all inside", const, -1., -np.inf),
             ("nan / inf", wild, 0.5, -np.inf), ("nan / inf floored", wild, 0.5, 0.), ("nan below a floor above iso", wild, -1., 0.),
             ("equal to iso", equal, 0.75, -np.inf)]
    for tag, sigma, iso, floor in cases:
        verts, faces = m.host_extract(sigma, iso, floor)   # (asserts the guard words around outputs and workspace)
        V, T = _predicted_counts(sigma, iso, floor)
        assert (len(verts), len(faces)) == (V, T), tag
        assert np.all(np.isfinite(verts)), tag
        assert faces.size == 0 or (faces.min() >= 0 and faces.max() < V), tag
        assert np.all(verts >= 0) and np.all(verts <= np.array(sigma.shape, F32) - 1), tag
    assert _predicted_counts(const, 3.5, -np.inf) == (0, 0) and _predicted_counts(const, -1., -np.inf) == (0, 0)
    assert _predicted_counts(wild, 0.5, -np.inf)[0] > 100
    # a NaN is outside whatever the floor: with floor 0 > iso = -1 every other point is inside
    inside, _, _ = m.crossing_edges(wild, -1., 0.)
    assert np.array_equal(inside, ~np.isnan(wild))
    # capacities that are too small: nothing at or beyond them is written, what is written is unchanged
    sigma = m.sphere_grid()
    verts, faces = m.host_extract(sigma, 0.)
    v2, f2, V, T = m.host_extract(sigma, 0., cap=(len(verts) - 1, len(faces) - 1))
    assert (V, T) == (len(verts), len(faces)) and np.array_equal(v2, verts[:-1]) and np.array_equal(f2, faces[:-1])
    # the output transform (p * scale + offset) + t * scale, two single-rounded fmas: against the float64 expression within one ulp of
    # the largest intermediate (|x| < 4: 2.4e-7 each, two of them) + the index-space bound of check 1 times the scale
    scale, off = 1. / 27, np.array([-.5, .25, 2.])
    v3, f3 = m.host_extract(sigma, 0., scale=scale, offset=tuple(off))
    _, p, ax = m.crossing_edges(sigma, 0.)
    pos, _, _ = m.vertex_positions_f64(sigma, 0., -np.inf, p, ax)
    want = pos * float(F32(scale)) + off
    assert np.abs(v3.astype(np.float64) - want).max() <= 2 * 2.4e-7 + (3e-7 + 1.2e-7 * 27) * scale and np.array_equal(f3, faces)
    # off the edge's axis it is one fma of the integer, exactly; a power-of-two scale and a centring offset keep the lower end exact
    k = np.arange(len(p))
    for c in range(3):
        sel = ax != c
        assert np.array_equal(v3[sel, c], (p[sel, c] * np.float64(F32(scale)) + off[c]).astype(F32))
    v4, _ = m.host_extract(sigma, 0., scale=1. / 32, offset=(-.5, -.5, -.5))
    t64 = (v4.astype(np.float64)[k, ax] + 0.5) * 32 - p[k, ax]
    assert np.abs(t64 - (pos[k, ax] - p[k, ax])).max() <= 32 * 2.0 ** -26 + 1.8e-7      # half an ulp of |x| < 0.5, and t's own error


def test_host_extractor_rejects_what_the_library_rejects():
    lib = m.host_lib()
    g = np.zeros((4, 4, 4), F32)
    ws, cnt = np.zeros(64, np.int32), np.zeros(2, np.int32)
    ok = lambda *a: lib.ref_mesh_count(g.ctypes.data, *a, ws.ctypes.data, cnt.ctypes.data)     # noqa: E731
    assert ok(4, 4, 4, 16, 4, -np.inf, 0.) == 0
    for bad in ((1, 4, 4, 16, 4, 0., 0.), (4, 1025, 4, 16, 4, 0., 0.), (4, 4, 4, -16, 4, 0., 0.), (4, 4, 4, 16, 4, 0., np.nan),
                (4, 4, 4, 16, 4, 0., np.inf), (4, 4, 4, 16, 4, np.nan, 0.), (4, 4, 4, 16, 4, np.inf, 0.)):
        assert ok(*bad) == -22, bad


# ----------------------------------------------------------------------------- 6. table, .ply
def test_table_regenerates_byte_for_byte():
    gen = m.gen_table_module()
    with open(os.path.join(m.CSRC, "mc_table.inc")) as f:
        assert f.read() == gen.render()
    lib = m.host_lib()
    for case in range(256):
        assert lib.ref_mc_case(case) == gen.pack(gen.TABLE[case])
    assert gen.TABLE[0] == [] and gen.TABLE[255] == []


def test_ply_round_trip_and_layout(tmp_path):
    from core.utils.mesh_io import read_ply, write_ply
    verts, faces = m.host_extract(m.sphere_grid(), 0., scale=1. / 27, offset=(-.5, -.5, -.5))
    path = str(tmp_path / "sphere.ply")
    write_ply(path, verts, faces)
    v, f = read_ply(path)
    assert v.dtype == np.float32 and f.dtype == np.int32 and v.tobytes() == verts.tobytes() and f.tobytes() == faces.tobytes()
    raw = open(path, "rb").read()
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
              "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % (len(verts), len(faces))).encode()
    assert raw.startswith(header) and len(raw) == len(header) + 12 * len(verts) + 13 * len(faces)
    body = raw[len(header):]
    assert body[:12] == verts[0].astype("<f4").tobytes()
    assert body[12 * len(verts):12 * len(verts) + 13] == b"\x03" + faces[0].astype("<i4").tobytes()
    empty = str(tmp_path / "empty.ply")
    write_ply(empty, np.zeros((0, 3), F32), np.zeros((0, 3), np.int32))
    v, f = read_ply(empty)
    assert v.shape == (0, 3) and f.shape == (0, 3) and v.dtype == np.float32 and f.dtype == np.int32
    assert b"element vertex 0\n" in open(empty, "rb").read() and b"element face 0\n" in open(empty, "rb").read()
    with pytest.raises(ValueError):
        write_ply(empty, verts, faces + len(verts))
    open(empty, "wb").write(raw[:-5])
    with pytest.raises(ValueError):
        read_ply(empty)


# ----------------------------------------------------------------------------- the library's host side
def test_library_checks_mesh_arguments_without_touching_the_gpu():
    from core import _hip
    lib = _hip.lib()
    assert lib.danbo_abi_version() == 9
    n = 65 * 33 * 17
    assert lib.danbo_mesh_workspace_bytes(65, 33, 17) == (4 * n + 15) // 16 * 16 + 8 * ((n + 255) // 256 + 1)
    assert lib.danbo_mesh_workspace_bytes(1024, 1024, 1024) == 4 * 2 ** 30 + 8 * (2 ** 22 + 1)        # 4 B per point + 8 B per chunk
    for dims in ((1, 8, 8), (8, 8, 1025), (0, 0, 0), (1024, 1024, 2048), (-4, 8, 8)):
        assert lib.danbo_mesh_workspace_bytes(*dims) == 0
    p = ctypes.c_void_p(4096)          # a non-null, aligned placeholder: every call below is rejected before it is looked at
    inf, nan = float("inf"), float("nan")
    good = dict(sigma=p, nx=8, ny=8, nz=8, sx=64, sy=8, floor=0., iso=1., ws=p)
    count = lambda **kw: (lambda a: lib.danbo_mesh_count(a["sigma"], a["nx"], a["ny"], a["nz"], a["sx"], a["sy"], a["floor"], a["iso"],     # noqa: E731
                                                         a["ws"], a.get("counts", p), None))({**good, **kw})
    extract = lambda **kw: (lambda a: lib.danbo_mesh_extract(a["sigma"], a["nx"], a["ny"], a["nz"], a["sx"], a["sy"], a["floor"], a["iso"],  # noqa: E731
                                                             a["ws"], a.get("scale", 1.), a.get("ox", 0.), 0., 0., a.get("verts", p),
                                                             a.get("cap_v", 4), a.get("tris", p), a.get("cap_t", 4), None))({**good, **kw})
    bad = [dict(sigma=None), dict(ws=None), dict(nx=1), dict(ny=1025), dict(nz=0), dict(sx=-1), dict(sy=-8), dict(iso=nan), dict(iso=inf),
           dict(floor=nan), dict(floor=inf), dict(sigma=ctypes.c_void_p(4098))]
    for kw in bad:
        assert count(**kw) == -22, kw
        assert extract(**kw) == -22, kw
    assert count(counts=None) == -22
    for kw in (dict(cap_v=-1), dict(cap_t=-1), dict(verts=None), dict(tris=None), dict(scale=nan), dict(ox=inf), dict(scale=inf)):
        assert extract(**kw) == -22, kw
    assert count(nx=2048) == -22 and extract(nz=-8) == -22


def test_wrapper_and_entry_points_know_the_mesh_path():
    import torch
    from core import hip_ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip_ops.marching_cubes(torch.zeros(4, 4, 4), 0.5)
    import run_render
    a = run_render.config_parser().parse_args(["--nerf_args", "x", "--ckptpath", "y", "--dataset", "synthetic", "--entry", "val",
                                               "--runname", "r", "--render_mesh"])
    assert a.mesh_threshold == 10.0
    a = run_render.config_parser().parse_args(["--nerf_args", "x", "--ckptpath", "y", "--dataset", "synthetic", "--entry", "val",
                                               "--runname", "r", "--render_mesh", "--mesh_threshold", "2.5"])
    assert a.mesh_threshold == 2.5
    from core.raycasters import RayCaster
    assert callable(RayCaster.render_mesh_surface)
    assert ROOT and "NNN.ply" in run_render.render_mesh.__doc__
