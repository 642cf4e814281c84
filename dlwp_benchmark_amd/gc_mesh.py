"""The icosphere file and the three graphs of the dlwpbench GraphCastNet as index arrays: numpy (scipy's k-d tree for the
neighbour searches), no dgl, no pymesh, no sklearn, and no import of the library -- the CPU tests use it as it is.

Reference: Graph in src/dlwpbench/models/graphcast/utils/graph.py (create_mesh_graph, create_g2m_graph, create_m2g_graph) with
add_edge_features / add_node_features / cell_to_adj / latlon2xyz of utils/graph_utils.py, and the file schema of
utils/icospheres.py (generate_and_save_icospheres, which needs pymesh; the reference ships no such file).  DGL is a container
there; its part is restated from its documentation: `to_bidirected` adds the reverse of every edge and drops duplicates.
tests/golden/make_graphcast_dlwp_golden.py runs the reference classes on a stub `dgl` and pins all three graphs.

The file: `order_i_vertices` [10 4^i + 2, 3], `order_i_faces` [20 4^i, 3], `order_i_face_centroid` (the mean of a face's three
vertices) for i = 0..level, plus the two empty lists `vertices` and `faces` the reference's writer emits -- its reader takes the
number of keys containing "faces", minus 2, as the finest order.  Subdivision APPENDS the edge midpoints, so the vertices of order i
are the first vertices of order i + 1: the multimesh indexes the finest vertices with the faces of every order.

The graphs (edge ORDER is ours, sorted by destination then source: the model only sums over edges):
* mesh   the multimesh on the finest vertices: the faces of all orders, each as three directed edges, both directions, no duplicates;
* g2m    grid node -> each of its 4 nearest mesh vertices that lies within 0.6 x the longest edge of the finest mesh;
* m2g    the three vertices of the face with the nearest centroid -> grid node.
Grid node u is point (u // width, u % width) of latitudes linspace(-90, 90, height) x longitudes linspace(-180, 180, width + 1)[1:].

Features are data a checkpoint was trained on and keep the reference's oddities:
* node features are cos(lat), sin(lon), cos(lon) with lat and lon in DEGREES handed to cos / sin as they are;
* positions are the fp32 numbers the reference holds (the file's vertices rounded to fp32; the grid's x, y, z formed in fp32 from
  fp32 angles, which puts the pole rows at cos(fp32(pi / 2)) = -4.4e-8 from the axis and so fixes their azimuth).
From those positions everything is formed in float64 and cast to fp32 once: the displacement source - destination rotated into the
destination's local frame (azimuth about z, then polar angle about y) and its norm, both over the largest norm of the graph.
"""
import json
from collections import namedtuple

import numpy as np

# src, dst [E] int32 (sorted by (dst, src)); edge_features [E, 4] fp32; num_src, num_dst
BiGraph = namedtuple("BiGraph", "src dst edge_features num_src num_dst")

_T = (1.0 + 5.0 ** 0.5) / 2.0
_ICO_VERTICES = [(-1, _T, 0), (1, _T, 0), (-1, -_T, 0), (1, -_T, 0), (0, -1, _T), (0, 1, _T), (0, -1, -_T), (0, 1, -_T),
                 (_T, 0, -1), (_T, 0, 1), (-_T, 0, -1), (-_T, 0, 1)]
_ICO_FACES = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
              (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]


def icospheres(level):
    """[(vertices [V, 3] float64 of unit norm, faces [F, 3] int64)] for the orders 0..level"""
    level = int(level)
    if level < 0:
        raise ValueError(f"level = {level} must be >= 0")
    v = np.asarray(_ICO_VERTICES, np.float64)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    verts, faces = [tuple(p) for p in v], [tuple(f) for f in _ICO_FACES]
    out = [(np.asarray(verts), np.asarray(faces, np.int64))]
    for _ in range(level):
        mid, new_faces = {}, []

        def midpoint(a, b):
            key = (a, b) if a < b else (b, a)
            if key not in mid:
                p = (np.asarray(verts[a]) + np.asarray(verts[b])) / 2.0
                verts.append(tuple(p / np.linalg.norm(p)))
                mid[key] = len(verts) - 1
            return mid[key]

        for a, b, c in faces:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            new_faces += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        faces = new_faces
        out.append((np.asarray(verts), np.asarray(faces, np.int64)))
    return out


def write_icospheres(path, level):
    """Write the orders 0..level in the JSON schema the reference reads (see the module docstring)."""
    doc = {"vertices": [], "faces": []}
    for i, (v, f) in enumerate(icospheres(level)):
        doc[f"order_{i}_vertices"] = v.tolist()
        doc[f"order_{i}_faces"] = f.tolist()
        doc[f"order_{i}_face_centroid"] = v[f].mean(axis=1).tolist()
    with open(path, "w") as fh:
        json.dump(doc, fh)


def load_icospheres(path):
    """(dict of arrays, finest order) by the reference's rule: the number of keys containing "faces", minus 2"""
    with open(path) as fh:
        doc = {k: (np.array(v) if isinstance(v, list) else v) for k, v in json.load(fh).items()}
    max_order = len([k for k in doc if "faces" in k]) - 2
    if max_order < 0 or any(f"order_{i}_{w}" not in doc for i in range(max_order + 1) for w in ("vertices", "faces", "face_centroid")):
        raise ValueError(f"{path}: not an icosphere file (order_i_vertices / _faces / _face_centroid for i = 0..level and the two "
                         "empty lists 'vertices', 'faces')")
    return doc, max_order


def grid_positions(height, width):
    """[height * width, 3] fp32: latlon2xyz of the reference's lat-lon grid, in fp32 step by step as there"""
    lat = np.linspace(-90, 90, int(height)).astype(np.float32)
    lon = np.linspace(-180, 180, int(width) + 1).astype(np.float32)[1:]
    lat, lon = (a.reshape(-1) for a in np.meshgrid(lat, lon, indexing="ij"))
    lat, lon = lat * np.float32(np.pi) / np.float32(180), lon * np.float32(np.pi) / np.float32(180)
    return np.stack([np.cos(lat) * np.cos(lon), np.cos(lat) * np.sin(lon), np.sin(lat)], axis=1).astype(np.float32)


def node_features(pos):
    """[N, 3] fp32: cos(lat), sin(lon), cos(lon) with both angles in degrees, as the reference forms them"""
    pos = np.asarray(pos, np.float32).astype(np.float64)
    lat, lon = np.degrees(np.arcsin(pos[:, 2])), np.degrees(np.arctan2(pos[:, 1], pos[:, 0]))
    return np.stack([np.cos(lat), np.sin(lon), np.cos(lon)], axis=1).astype(np.float32)


def edge_features(src, dst, src_pos, dst_pos):
    """[E, 4] fp32: (source - destination) in the destination's local frame and its norm, over the largest norm"""
    s = np.asarray(src_pos, np.float32).astype(np.float64)[np.asarray(src, np.int64)]
    d = np.asarray(dst_pos, np.float32).astype(np.float64)[np.asarray(dst, np.int64)]
    lat, lon = np.arcsin(d[:, 2]), np.arctan2(d[:, 1], d[:, 0])
    az = np.where(lon >= 0.0, 2 * np.pi - lon, -lon)
    pol = np.where(lat >= 0.0, lat, 2 * np.pi + lat)

    def rotate(p):
        c, sn = np.cos(az), np.sin(az)
        x, y, z = c * p[:, 0] - sn * p[:, 1], sn * p[:, 0] + c * p[:, 1], p[:, 2]
        c, sn = np.cos(pol), np.sin(pol)
        return np.stack([c * x + sn * z, y, -sn * x + c * z], axis=1)

    disp = rotate(s) - rotate(d)
    norm = np.linalg.norm(disp, axis=1, keepdims=True)
    return np.ascontiguousarray(np.concatenate([disp, norm], axis=1) / norm.max(), dtype=np.float32)


def _sorted(src, dst):
    """the edges sorted by (dst, src)"""
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    key = np.lexsort((src, dst))
    return src[key], dst[key]


def build_graphs(ico, max_order, height, width):
    """-> dict(mesh=BiGraph, g2m=BiGraph, m2g=BiGraph, mesh_node_features [V, 3] fp32) for a height x width grid on the icospheres
    of load_icospheres"""
    from scipy.spatial import cKDTree
    height, width = int(height), int(width)
    if height < 2 or width < 1:
        raise ValueError(f"a {height} x {width} lat-lon grid: at least 2 latitudes and 1 longitude are needed")
    vert = np.asarray(ico[f"order_{max_order}_vertices"], np.float64)
    faces = np.asarray(ico[f"order_{max_order}_faces"], np.int64)
    nv, ng = len(vert), height * width
    grid = grid_positions(height, width)
    # the multimesh
    cells = np.concatenate([np.asarray(ico[f"order_{i}_faces"], np.int64) for i in range(max_order + 1)])
    a, b = cells[:, [0, 1, 2]].reshape(-1), cells[:, [1, 2, 0]].reshape(-1)
    if a.max() >= nv:
        raise ValueError("the faces of a coarser order name vertices beyond the finest order's")
    key = np.unique(np.concatenate([b * nv + a, a * nv + b]))
    dst, src = key // nv, key % nv
    mesh = BiGraph(src.astype(np.int32), dst.astype(np.int32), edge_features(src, dst, vert, vert), nv, nv)
    # grid -> mesh: the 4 nearest vertices within 0.6 x the longest finest edge
    tri = vert[faces]
    edge_len = max(np.linalg.norm(tri[:, i] - tri[:, j], axis=1).max() for i, j in ((0, 1), (0, 2), (1, 2)))
    dist, idx = cKDTree(vert).query(grid.astype(np.float64), k=min(4, nv))
    dist, idx = dist.reshape(ng, -1), idx.reshape(ng, -1)
    keep = dist <= 0.6 * edge_len
    src, dst = _sorted(np.repeat(np.arange(ng), keep.shape[1])[keep.reshape(-1)], idx.reshape(-1)[keep.reshape(-1)])
    if len(src) == 0:
        raise ValueError(f"no grid point of the {height} x {width} grid lies within 0.6 x {edge_len:.4f} of a mesh vertex")
    g2m = BiGraph(src.astype(np.int32), dst.astype(np.int32), edge_features(src, dst, grid, vert), ng, nv)
    # mesh -> grid: the vertices of the face with the nearest centroid
    _, near = cKDTree(np.asarray(ico[f"order_{max_order}_face_centroid"], np.float64)).query(grid.astype(np.float64), k=1)
    src, dst = _sorted(faces[near.reshape(-1)].reshape(-1), np.repeat(np.arange(ng), 3))
    m2g = BiGraph(src.astype(np.int32), dst.astype(np.int32), edge_features(src, dst, vert, grid), nv, ng)
    return dict(mesh=mesh, g2m=g2m, m2g=m2g, mesh_node_features=node_features(vert))
