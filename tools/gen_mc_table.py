"""Generates danbo-pytorch_amd/csrc/mc_table.inc: the 256-case triangle table of the isosurface extraction (csrc/mesh_math.hpp,
csrc/k_mesh.hip).  Nothing is copied from an existing table; the construction is watertight by design:

  * cube corner c = a + 2b + 4c' sits at (a, b, c'); a case is the 8-bit mask of INSIDE corners;
  * cube edge e = 4 * axis + r: it runs along `axis` from the corner whose two other coordinates are (r & 1, r >> 1) (in the order
    of the remaining axes) -- EDGE_CORNER below; the edge's vertex is owned by that lower corner;
  * on every cube face the crossing edges (ends differ in inside-ness) are joined by directed segments: two crossings -> one
    segment; four crossings (the corners alternate) -> two segments, each cutting off one INSIDE corner.  The rule reads the four
    corner signs of the face only, so the two cells that share a face draw the same segments there.  A segment is directed so that,
    seen from outside the cube, an inside corner lies on its RIGHT side: the triangles' normals then point from inside (high
    density) to outside, and the signed volume of a closed surface around a dense region is positive;
  * every crossing edge gets exactly one outgoing and one incoming segment; following them gives closed loops, each loop is
    fan-triangulated.  A fan diagonal that lies in a cube face (possible only in a face with four crossings) can coincide with
    an edge of the neighbouring cell's triangles: the fan's apex is the loop position with the fewest such diagonals (the first
    of them in loop order, the loop starting at its lowest edge).

At most 5 triangles per case, 820 over the 256 cases.  One 64-bit word per case: bits 0-3 = the triangle count, bits 4 + 4n ..
7 + 4n = the cube edge of the n-th triangle corner (n = 3 * triangle + corner).

    python tools/gen_mc_table.py            # rewrites csrc/mc_table.inc
"""
import os

CORNER = [(c & 1, (c >> 1) & 1, (c >> 2) & 1) for c in range(8)]


def edge_corner(e):
    """lower corner (as a corner number) of cube edge e"""
    ax, r = e >> 2, e & 3
    p = [0, 0, 0]
    others = [a for a in range(3) if a != ax]
    p[others[0]], p[others[1]] = r & 1, r >> 1
    return p[0] + 2 * p[1] + 4 * p[2]


EDGE_CORNER = [edge_corner(e) for e in range(12)]
EDGE_ENDS = [(EDGE_CORNER[e], EDGE_CORNER[e] + (1 << (e >> 2))) for e in range(12)]
EDGE_ID = {ends: e for e, ends in enumerate(EDGE_ENDS)}


def eid(a, b):
    return EDGE_ID[(min(a, b), max(a, b))]


def faces():
    """the six faces as (corners in cyclic order, outward normal)"""
    out = []
    for ax in range(3):
        for v in (0, 1):
            cs = [c for c in range(8) if CORNER[c][ax] == v]
            cyc, rest = [cs[0]], cs[1:]
            while rest:
                n = [r for r in rest if bin(r ^ cyc[-1]).count("1") == 1][0]
                cyc.append(n)
                rest.remove(n)
            nrm = [0, 0, 0]
            nrm[ax] = 1 if v else -1
            out.append((cyc, tuple(nrm)))
    return out


FACES = faces()


def _mid2(e):
    """twice the midpoint of edge e (integers)"""
    a, b = EDGE_ENDS[e]
    return tuple(CORNER[a][i] + CORNER[b][i] for i in range(3))


def _cross(u, v):
    return (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])


def _on_a_face(e0, e1):
    cs = set(EDGE_ENDS[e0]) | set(EDGE_ENDS[e1])
    return any(cs <= set(cyc) for cyc, _ in FACES)


def case_triangles(case):
    """-> list of (e0, e1, e2) cube-edge triples"""
    ins = [(case >> c) & 1 for c in range(8)]
    nxt = {}

    def segment(nrm, a, b, corner):
        ma, mb = _mid2(a), _mid2(b)
        d = tuple(mb[i] - ma[i] for i in range(3))
        w = tuple(2 * CORNER[corner][i] - ma[i] for i in range(3))
        side = sum(n * c for n, c in zip(nrm, _cross(d, w)))       # > 0: the inside corner is on the left of a -> b (seen from outside)
        assert side != 0
        if side > 0:
            a, b = b, a
        assert a not in nxt, (case, a)
        nxt[a] = b

    for cyc, nrm in FACES:
        cross = [i for i in range(4) if ins[cyc[i]] != ins[cyc[(i + 1) % 4]]]
        if len(cross) == 2:
            corner = [c for c in cyc if ins[c]][0]
            segment(nrm, eid(cyc[cross[0]], cyc[(cross[0] + 1) % 4]), eid(cyc[cross[1]], cyc[(cross[1] + 1) % 4]), corner)
        elif len(cross) == 4:
            for i in range(4):
                if ins[cyc[i]]:
                    segment(nrm, eid(cyc[i], cyc[(i + 1) % 4]), eid(cyc[i], cyc[(i - 1) % 4]), cyc[i])
    n_cross = sum(ins[a] != ins[b] for a, b in EDGE_ENDS)
    assert len(nxt) == n_cross and sorted(nxt.values()) == sorted(nxt)      # one outgoing and one incoming segment per crossing edge
    seen, tris = set(), []
    for s in sorted(nxt):
        if s in seen:
            continue
        loop, cur = [s], nxt[s]
        seen.add(s)
        while cur != s:
            loop.append(cur)
            seen.add(cur)
            cur = nxt[cur]
        assert len(loop) >= 3
        n = len(loop)
        in_face = [sum(_on_a_face(loop[r], loop[(r + i) % n]) for i in range(2, n - 1)) for r in range(n)]
        r = in_face.index(min(in_face))
        loop = loop[r:] + loop[:r]
        for i in range(1, n - 1):
            tris.append((loop[0], loop[i], loop[i + 1]))
    return tris


TABLE = [case_triangles(m) for m in range(256)]


def pack(tris):
    assert len(tris) <= 5
    w = len(tris)
    for n, e in enumerate(e for t in tris for e in t):
        w |= e << (4 + 4 * n)
    return w


def render():
    lines = ["// generated by tools/gen_mc_table.py -- do not edit.  One word per case (8-bit mask of inside corners, corner = a + 2b + 4c):",
             "// bits 0-3 = triangles, bits 4 + 4n .. 7 + 4n = cube edge (4 * axis + r) of triangle corner n.  %d triangles in all."
             % sum(len(t) for t in TABLE)]
    for r in range(0, 256, 4):
        lines.append(" ".join("0x%016xull," % pack(TABLE[m]) for m in range(r, r + 4)))
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "danbo-pytorch_amd", "csrc", "mc_table.inc")
    with open(out, "w") as f:
        f.write(render())
    print("wrote", out, "max triangles per case", max(len(t) for t in TABLE), "total", sum(len(t) for t in TABLE))
