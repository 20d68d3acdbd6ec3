"""Binary .ply files of triangle meshes, numpy only: the layout trimesh's `mesh.export('x.ply')` writes (the reference's
run_render.py:1280-1281), so whatever read the reference's `meshes/NNN.ply` reads these."""
import numpy as np

_XYZ = [('x', '<f4'), ('y', '<f4'), ('z', '<f4')]
_NORMAL = [('nx', '<f4'), ('ny', '<f4'), ('nz', '<f4')]
_COLOR = [('red', 'u1'), ('green', 'u1'), ('blue', 'u1'), ('alpha', 'u1')]
_VERTEX = np.dtype(_XYZ)
_FACE = np.dtype([('n', 'u1'), ('v', '<i4', (3,))])
_PLY_TYPE = {'<f4': 'float', 'u1': 'uchar'}


def _vertex_dtype(normals, colors):
    return np.dtype(_XYZ + (_NORMAL if normals else []) + (_COLOR if colors else []))


def ply_header(n_verts, n_faces, normals=False, colors=False):
    props = "".join(f"property {_PLY_TYPE[t]} {name}\n" for name, t in _XYZ + (_NORMAL if normals else []) + (_COLOR if colors else []))
    return ("ply\nformat binary_little_endian 1.0\n"
            f"element vertex {n_verts}\n{props}"
            f"element face {n_faces}\nproperty list uchar int vertex_indices\nend_header\n")


def _host(x, dtype):
    return np.ascontiguousarray(np.asarray(x.cpu() if hasattr(x, 'cpu') else x, dtype=dtype))


def write_ply(path, verts, faces, normals=None, colors=None):
    """verts [V,3] float32, faces [T,3] int32 (arrays or tensors); a mesh without a face is a valid file with two zero counts.
    normals [V,3] float32 and colors [V,3] uint8, when given, extend the vertex record to `x y z [nx ny nz] [red green blue alpha]`
    (float, float, uchar; alpha = 255): the order and the types of trimesh's exporter.  trimesh is not a dependency, so that
    layout is pinned by the header text alone (tests/test_mesh_normals.py), not against a file trimesh wrote.  Without the two
    arguments the file is the one this function has always written, byte for byte."""
    verts = _host(verts, '<f4').reshape(-1, 3)
    faces = _host(faces, '<i4').reshape(-1, 3)
    if len(faces) and (faces.min() < 0 or faces.max() >= len(verts)):
        raise ValueError("write_ply: a face index is outside the vertex array")
    vrec = np.empty(len(verts), _vertex_dtype(normals is not None, colors is not None))
    vrec['x'], vrec['y'], vrec['z'] = verts.T
    if normals is not None:
        normals = _host(normals, '<f4')
        if normals.shape != verts.shape:
            raise ValueError(f"write_ply: normals {normals.shape} do not match the {len(verts)} vertices")
        vrec['nx'], vrec['ny'], vrec['nz'] = normals.T
    if colors is not None:
        colors = _host(colors, 'u1')
        if colors.shape != verts.shape:
            raise ValueError(f"write_ply: colors {colors.shape} do not match the {len(verts)} vertices")
        vrec['red'], vrec['green'], vrec['blue'] = colors.T
        vrec['alpha'] = 255
    rec = np.empty(len(faces), _FACE)
    rec['n'], rec['v'] = 3, faces
    with open(path, 'wb') as f:
        f.write(ply_header(len(verts), len(faces), normals is not None, colors is not None).encode('ascii'))
        f.write(vrec.tobytes())
        f.write(rec.tobytes())


def read_ply_attrs(path):
    """-> verts [V,3] float32, faces [T,3] int32, {'normals': [V,3] float32, 'colors': [V,3] uint8} with the entries the file
    holds -- of a file in one of the four layouts write_ply writes"""
    with open(path, 'rb') as f:
        data = f.read()
    marker = b"end_header\n"
    if marker not in data:
        raise ValueError(f"read_ply: {path} has no ply header")
    end = data.index(marker) + len(marker)
    try:
        header = data[:end].decode('ascii')
        counts = {}
        for line in header.split("\n"):
            w = line.split()
            if len(w) == 3 and w[0] == 'element':
                counts[w[1]] = int(w[2])
    except ValueError:
        raise ValueError(f"read_ply: {path} has no readable ply header") from None
    V, T = counts.get('vertex', -1), counts.get('face', -1)
    layout = [(n, c) for n in (False, True) for c in (False, True) if header == ply_header(V, T, n, c)]
    if not layout:
        raise ValueError(f"read_ply: {path} is not in the binary_little_endian float x/y/z [nx/ny/nz] [uchar rgba] + uchar/int "
                         "triangle-list layout")
    has_n, has_c = layout[0]
    vdt = _vertex_dtype(has_n, has_c)
    if len(data) != end + V * vdt.itemsize + T * _FACE.itemsize:
        raise ValueError(f"read_ply: {path} is truncated or longer than its header says")
    vrec = np.frombuffer(data, vdt, V, end)
    rec = np.frombuffer(data, _FACE, T, end + V * vdt.itemsize)
    if np.any(rec['n'] != 3):
        raise ValueError(f"read_ply: {path} holds polygons other than triangles")
    cols = lambda names, dt: np.stack([vrec[n] for n in names], -1).astype(dt).reshape(-1, 3)  # noqa: E731
    attrs = {}
    if has_n:
        attrs['normals'] = cols(('nx', 'ny', 'nz'), np.float32)
    if has_c:
        attrs['colors'] = cols(('red', 'green', 'blue'), np.uint8)
    return cols(('x', 'y', 'z'), np.float32), rec['v'].astype(np.int32).reshape(-1, 3), attrs


def read_ply(path):
    """-> verts [V,3] float32, faces [T,3] int32 of a file in one of the layouts write_ply writes"""
    return read_ply_attrs(path)[:2]
