"""Binary .ply files of triangle meshes, numpy only: the layout trimesh's `mesh.export('x.ply')` writes (the reference's
run_render.py:1280-1281), so whatever read the reference's `meshes/NNN.ply` reads these."""
import numpy as np

_VERTEX = np.dtype([('x', '<f4'), ('y', '<f4'), ('z', '<f4')])
_FACE = np.dtype([('n', 'u1'), ('v', '<i4', (3,))])


def ply_header(n_verts, n_faces):
    return ("ply\nformat binary_little_endian 1.0\n"
            f"element vertex {n_verts}\nproperty float x\nproperty float y\nproperty float z\n"
            f"element face {n_faces}\nproperty list uchar int vertex_indices\nend_header\n")


def write_ply(path, verts, faces):
    """verts [V,3] float32, faces [T,3] int32 (arrays or tensors); a mesh without a face is a valid file with two zero counts"""
    verts = np.ascontiguousarray(np.asarray(verts.cpu() if hasattr(verts, 'cpu') else verts, dtype='<f4')).reshape(-1, 3)
    faces = np.ascontiguousarray(np.asarray(faces.cpu() if hasattr(faces, 'cpu') else faces, dtype='<i4')).reshape(-1, 3)
    if len(faces) and (faces.min() < 0 or faces.max() >= len(verts)):
        raise ValueError("write_ply: a face index is outside the vertex array")
    rec = np.empty(len(faces), _FACE)
    rec['n'], rec['v'] = 3, faces
    with open(path, 'wb') as f:
        f.write(ply_header(len(verts), len(faces)).encode('ascii'))
        f.write(verts.view(_VERTEX).tobytes())
        f.write(rec.tobytes())


def read_ply(path):
    """-> verts [V,3] float32, faces [T,3] int32 of a file in the layout write_ply writes"""
    with open(path, 'rb') as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    header = data[:end].decode('ascii')
    counts = {}
    for line in header.split("\n"):
        w = line.split()
        if len(w) == 3 and w[0] == 'element':
            counts[w[1]] = int(w[2])
    if header != ply_header(counts.get('vertex', -1), counts.get('face', -1)):
        raise ValueError(f"read_ply: {path} is not in the binary_little_endian float x/y/z + uchar/int triangle-list layout")
    V, T = counts['vertex'], counts['face']
    verts = np.frombuffer(data, _VERTEX, V, end)
    rec = np.frombuffer(data, _FACE, T, end + V * _VERTEX.itemsize)
    if len(data) != end + V * _VERTEX.itemsize + T * _FACE.itemsize or np.any(rec['n'] != 3):
        raise ValueError(f"read_ply: {path} is truncated or holds polygons other than triangles")
    return (np.stack([verts['x'], verts['y'], verts['z']], -1).astype(np.float32).reshape(-1, 3),
            rec['v'].astype(np.int32).reshape(-1, 3))
