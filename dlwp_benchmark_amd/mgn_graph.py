"""The fixed meshes of the MeshGraphNet and GraphCastNS baselines as index arrays: numpy only (scipy for the Delaunay
triangulation), no networkx, no DGL, and no import of the library -- the CPU tests use it as it is.

Reference: MeshGraphNet.create_grid_2d_graph / create_grid_2d_graph_8stencil / create_delaunay_graph / create_edge_features in
src/nsbench/models/mgn/meshgraphnet.py:231-341 and src/dlwpbench/models/mgn/meshgraphnet.py:233-345, which build a networkx graph
and hand it to `dgl.to_bidirected(dgl.from_networkx(graph))`.  DGL is not installed where this was written, so its part is
RESTATED from its documentation, not executed:
* `from_networkx` relabels the nodes to consecutive integers in sorted label order (and gives every undirected edge both directions);
* `to_bidirected` adds the reverse of every edge and drops duplicates;
* `batch` offsets the node ids of sample b by b * num_nodes.
tests/golden/make_mgn_golden.py runs the reference classes on a stub `dgl` with exactly this behaviour.
GraphCastNS's mesh (build_nhop_grid: the periodic grid plus n-hop shortcuts, GraphCastNetNS.create_grid_2d_graph /
create_edge_features in src/nsbench/models/graphcast/graph_cast_net_ns.py:252-312, which walk a networkx graph node by node and
edge by edge) is restated the same way and pinned by tests/golden/make_graphcast_ns_golden.py.

Node u is grid point (u // width, u % width): the order of the models' "(b h w) d" rows.  The edge ORDER is ours (the model only
sums over edges): sorted by destination, then source, so the in-edges of a node are consecutive.

The edge features are data a checkpoint was trained on and are reproduced with their oddities:
* the coordinates of node u are taken as (u // HEIGHT, u % width), which is not the grid point where height != width;
* the wrap-around fix rewrites only the differences +-(height - 1) and +-(width - 1), one rule after the other on both components;
* the 8-stencil's third feature is sqrt(|dx| + |dy|) divided by its largest value;
* the 8-stencil's diagonal neighbours are taken modulo HEIGHT on both axes, whatever `periodic` says: on height < width this adds
  edges from the columns >= height back into the first ones (kept); on height > width the reference creates node labels
  outside the grid, which is refused here.
"""
from collections import namedtuple

import numpy as np

GRAPH_TYPES = ("grid_2d", "grid_2d_8stencil", "delaunay")
EDGE_FEATURES = {"grid_2d": 2, "grid_2d_8stencil": 3, "delaunay": 2}

# src, dst [E] int32 (directed, both directions, no duplicates, sorted by (dst, src)); edge_features [E, 2 | 3] fp32;
# in_ptr [N + 1], in_eid [E]: edge ids grouped by destination; out_ptr [N + 1], out_eid [E]: grouped by source (int32)
Graph = namedtuple("Graph", "src dst edge_features num_nodes in_ptr in_eid out_ptr out_eid")


def _periodic_pair(periodic):
    try:
        pr, pc = periodic
    except TypeError:
        pr = pc = periodic
    return bool(pr), bool(pc)


def build_csr(src, dst, num_nodes):
    """(in_ptr, in_eid, out_ptr, out_eid), int32: edge ids grouped by destination / by source, ascending inside a group."""
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    out = []
    for key in (dst, src):
        eid = np.argsort(key, kind="stable")
        ptr = np.zeros(num_nodes + 1, np.int64)
        np.cumsum(np.bincount(key, minlength=num_nodes), out=ptr[1:])
        out += [ptr.astype(np.int32), eid.astype(np.int32)]
    return tuple(out)


def _grid_pairs(height, width, periodic):
    """undirected edges of networkx.grid_2d_graph(height, width, periodic) as label pairs ((i, j), (i', j'))"""
    pr, pc = _periodic_pair(periodic)
    i, j = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
    pairs = [(i[1:], j[1:], i[:-1], j[:-1]), (i[:, 1:], j[:, 1:], i[:, :-1], j[:, :-1])]
    if pr and height > 2:
        pairs.append((i[0], j[0], i[-1], j[-1]))
    if pc and width > 2:
        pairs.append((i[:, 0], j[:, 0], i[:, -1], j[:, -1]))
    return [tuple(a.reshape(-1) for a in p) for p in pairs]


def _delaunay_pairs(height, width, periodic, cylinder):
    """undirected edges of the reference's triangulation after its merges, as pairs of merged POINT labels"""
    from scipy.spatial import Delaunay
    rows = height if cylinder else height + 1
    if not periodic:
        raise ValueError("graph_type 'delaunay' needs periodic=True: without the merge of the last column (and row) the reference's "
                         f"graph has {rows * (width + 1)} nodes for a {height} x {width} grid")
    # points in the reference's order (x fastest, fp32 coordinates): the grid is degenerate for a triangulation, so which
    # diagonal a cell gets depends on it
    y, x = np.divmod(np.arange(rows * (width + 1)), width + 1)
    simplices = Delaunay(np.stack([x.astype(np.float32), y.astype(np.float32)], axis=1)).simplices
    # the last column is the first one again, and (both axes closed) the last row the first
    q, r = np.divmod(simplices, width + 1)
    simplices = (q % height) * (width + 1) + r % width
    a = np.concatenate([simplices[:, 0], simplices[:, 1], simplices[:, 2]])
    b = np.concatenate([simplices[:, 1], simplices[:, 2], simplices[:, 0]])
    return a, b


def edge_features(src, dst, height, width, add_distance):
    """create_edge_features of the reference on int64 / float32 arithmetic (bit for bit: integers, one fp32 sqrt, one fp32 division)"""
    u, v = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    normal = np.stack([v // height - u // height, v % width - u % width], axis=1)
    for old, new in ((height - 1, -1), (width - 1, -1), (-(height - 1), 1), (-(width - 1), 1)):
        normal[normal == old] = new
    feats = normal.astype(np.float32)
    if add_distance:
        dist = np.sqrt(np.abs(normal).sum(axis=1).astype(np.float32))
        feats = np.concatenate([feats, (dist / dist.max())[:, None]], axis=1)
    return np.ascontiguousarray(feats, dtype=np.float32)


def build_graph(graph_type, height, width, periodic=True, cylinder=False):
    """The reference's mesh for an H x W grid -> Graph.  graph_type: "grid_2d", "grid_2d_8stencil" or "delaunay"; periodic: a bool
    or a (rows, columns) pair as networkx takes it.  cylinder (delaunay only): the dlwpbench form, which triangulates H x (W + 1)
    points and closes the longitude only; the nsbench form triangulates (H + 1) x (W + 1) points and closes both axes."""
    height, width = int(height), int(width)
    if height < 1 or width < 1:
        raise ValueError(f"a {height} x {width} grid has no nodes")
    if graph_type not in GRAPH_TYPES:
        raise ValueError(f"graph_type is '{graph_type}' but should be any of {list(GRAPH_TYPES)}.")
    n = height * width
    if graph_type == "delaunay":
        a, b = _delaunay_pairs(height, width, periodic, cylinder)
        # merged point label y (W + 1) + x, x < W, y < H  ->  rank in sorted label order = y W + x
        a, b = (a // (width + 1)) * width + a % (width + 1), (b // (width + 1)) * width + b % (width + 1)
        if a.max() >= n or b.max() >= n or len(np.unique(np.concatenate([a, b]))) != n:
            raise ValueError(f"the triangulation of a {height} x {width} grid does not cover its {n} nodes")
    else:
        pairs = _grid_pairs(height, width, periodic)
        if graph_type == "grid_2d_8stencil":
            if height > width:
                raise ValueError(f"grid_2d_8stencil on a {height} x {width} grid: the reference takes the diagonal neighbours modulo "
                                 "the height on both axes, which names columns outside a grid with height > width")
            i, j = (x.reshape(-1) for x in np.meshgrid(np.arange(height), np.arange(width), indexing="ij"))
            for di, dj in ((-1, 1), (1, 1), (1, -1), (-1, -1)):
                pairs.append((i, j, (i + di) % height, (j + dj) % height))
        a = np.concatenate([p[0] * width + p[1] for p in pairs])
        b = np.concatenate([p[2] * width + p[3] for p in pairs])
    # both directions, duplicates dropped, sorted by (dst, src)
    key = np.unique(np.concatenate([b * n + a, a * n + b]).astype(np.int64))
    dst, src = key // n, key % n
    feats = edge_features(src, dst, height, width, graph_type == "grid_2d_8stencil")
    return Graph(src.astype(np.int32), dst.astype(np.int32), feats, n, *build_csr(src, dst, n))


def nhop_edge_features(src, dst, height, width, nhop_neighbors):
    """GraphCastNetNS.create_edge_features of the reference: [dir_y, dir_x, dist] per directed edge.  The coordinates are
    (u // HEIGHT, u % width) as there; the four wrap-around assignments run one after the other on BOTH components (on a small grid
    a later one rewrites what an earlier one set); dist is the distance on the 1-hop torus (true grid coordinates) over max(nhop),
    formed in float64 and rounded to fp32 as there."""
    u, v = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    m = int(max(nhop_neighbors))
    normal = np.stack([v // height - u // height, v % width - u % width], axis=1)
    normal[normal >= height - 1 - m] = -1
    normal[normal >= width - 1 - m] = -1
    normal[normal <= -(height - 1 - m)] = 1
    normal[normal <= -(width - 1 - m)] = 1
    normal = normal.clip(-1, 1)
    di, dj = np.abs(v // width - u // width), np.abs(v % width - u % width)
    dist = (np.minimum(di, height - di) + np.minimum(dj, width - dj)) / float(m)
    return np.ascontiguousarray(np.concatenate([normal.astype(np.float64), dist[:, None]], axis=1), dtype=np.float32)


def build_nhop_grid(height, width, nhop_neighbors=(2,)):
    """The mesh of the reference's GraphCastNetNS (src/nsbench/models/graphcast/graph_cast_net_ns.py:252-312) -> Graph with
    edge_features [E, 3]: the periodic height x width 4-neighbour grid (always periodic) plus "n-hop" shortcuts.  Every node
    (i, j) with a multiple of some nhop value on each axis gets an undirected edge to every node of its row or column whose torus
    distance d is one of the nhop values and d <= max(nhop) - max(max(i, j) % nhop); then both directions, duplicates dropped."""
    height, width = int(height), int(width)
    nhop = np.unique(np.asarray(list(nhop_neighbors), np.int64))
    if height < 3 or width < 3:
        raise ValueError(f"the periodic n-hop grid needs at least 3 x 3 nodes, not {height} x {width}")
    if len(nhop) == 0 or nhop[0] < 1:
        raise ValueError(f"nhop_neighbors must be positive hop counts, not {list(nhop_neighbors)}")
    n = height * width
    pairs = _grid_pairs(height, width, True)
    a = [p[0] * width + p[1] for p in pairs]
    b = [p[2] * width + p[3] for p in pairs]
    i, j = (x.reshape(-1) for x in np.meshgrid(np.arange(height), np.arange(width), indexing="ij"))
    listed = ((i[:, None] % nhop) == 0).any(axis=1) & ((j[:, None] % nhop) == 0).any(axis=1)
    cutoff = nhop[-1] - (np.maximum(i, j)[:, None] % nhop).max(axis=1)
    for d in nhop:
        sel = listed & (d <= cutoff)
        si, sj = i[sel], j[sel]
        # a node of the same row (column) at torus distance d exists only while 2 d <= the row's (column's) length
        for ok, ti, tj in ((2 * d <= width, si, (sj + d) % width), (2 * d <= width, si, (sj - d) % width),
                           (2 * d <= height, (si + d) % height, sj), (2 * d <= height, (si - d) % height, sj)):
            if ok:
                a.append(si * width + sj)
                b.append(ti * width + tj)
    a, b = np.concatenate(a), np.concatenate(b)
    key = np.unique(np.concatenate([b * n + a, a * n + b]).astype(np.int64))
    dst, src = key // n, key % n
    feats = nhop_edge_features(src, dst, height, width, nhop)
    return Graph(src.astype(np.int32), dst.astype(np.int32), feats, n, *build_csr(src, dst, n))


def check_range(src, dst, num_nodes):
    """Raise ValueError unless src and dst are equally many node ids in [0, num_nodes)."""
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    E = len(src)
    if len(dst) != E or (E and (src.min() < 0 or dst.min() < 0 or src.max() >= num_nodes or dst.max() >= num_nodes)):
        raise ValueError(f"edge endpoints must be {E} pairs of node ids in [0, {num_nodes})")


def check_csr(src, dst, num_nodes, in_ptr, in_eid, out_ptr, out_eid):
    """Raise ValueError unless the indices are in range and the two CSR forms describe exactly the edges (src, dst)."""
    check_range(src, dst, num_nodes)
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    E = len(src)
    for name, ptr, eid, key in (("in", in_ptr, in_eid, dst), ("out", out_ptr, out_eid, src)):
        ptr, eid = np.asarray(ptr, np.int64), np.asarray(eid, np.int64)
        if len(ptr) != num_nodes + 1 or len(eid) != E or ptr[0] != 0 or ptr[-1] != E or (np.diff(ptr) < 0).any():
            raise ValueError(f"{name}_ptr must rise from 0 to {E} over {num_nodes + 1} entries and {name}_eid hold {E} edge ids")
        if E and (eid.min() < 0 or eid.max() >= E or len(np.unique(eid)) != E):
            raise ValueError(f"{name}_eid must be a permutation of the {E} edge ids")
        if E and not np.array_equal(key[eid], np.repeat(np.arange(num_nodes), np.diff(ptr))):
            raise ValueError(f"{name}_ptr / {name}_eid do not group the edges by their {'destination' if name == 'in' else 'source'}")
